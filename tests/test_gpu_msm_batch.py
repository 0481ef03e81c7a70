"""The batched MSM (zkt_*_msm_batch_submit / _collect / _dev: k scalar vectors over one resident base set in one pass) against python integers,
for G1, G2 and secp256k1.

Bases are k_i * G with known k_i (a prefix of one shared set per group), so the expected point of vector v is (sum k_i s_vi mod order) * G, computed
from python integers alone; every out[v] is also compared with zkt_*_msm_dev of vector v alone, which it must equal bit for bit.  The constructed
vectors come from tests/msm_batch_model.py, whose claims (which bucket of which set they fill) tests/test_msm_batch_model.py checks on the CPU."""
import ctypes, importlib, os, subprocess, sys
import numpy as np
import pytest
import msm_plan_model as M
import msm_batch_model as B
from zkt_testlib import G1W, G2W, G1_GEN, G2_GEN, SECP_GEN, py_g1_mul, py_g2_mul, py_secp_mul, g1_arr, g2_arr, secp_arr, to_abi_g2, ptr

pytestmark = pytest.mark.gpu
if os.environ.get("ZKT_MSM_C"):
    pytest.skip("a forced window width invalidates the bucket claims of these cases", allow_module_level=True)
zk = importlib.import_module("zk-toolkit_amd")

W = {"g1": G1W, "g2": G2W, "secp": 9}
PW = {"g1": zk.G1_PARTIAL_WORDS, "g2": zk.G2_PARTIAL_WORDS, "secp": zk.SECP_PARTIAL_WORDS}
GEN = {"g1": g1_arr([G1_GEN]), "g2": g2_arr([G2_GEN]), "secp": secp_arr([SECP_GEN])}
SHAPE = zk.ZKT_ERR_SHAPE


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _point(group, tot):
    if group == "g1":
        return g1_arr([py_g1_mul(G1_GEN, tot)])
    if group == "secp":
        return secp_arr([py_secp_mul(SECP_GEN, tot)])
    (x1, x0), (y1, y0) = G2_GEN
    pt = py_g2_mul(((x0, x1), (y0, y1)), tot)
    return g2_arr([None if pt is None else to_abi_g2(pt)])


def _fn(L, group, name):
    return getattr(L, f"zkt_{group}_{name}")


# ---- one shared base set per group (k_i * G, i < POOL_N), one live handle at a time, references computed once ---------------------------
_bases, _handle, _want, _single = {}, {}, {}, {}


def _base_set(L, group):
    import torch
    if group not in _bases:
        n = B.POOL_N
        ks = np.ascontiguousarray(M.random_ks(M.K_SEED)[:n])
        if group == "secp":                                              # secp256k1 has no device form of the batch product
            host = np.zeros((n, 9), np.uint64)
            zk.check(L.zkt_secp_mul_batch(ptr(np.repeat(GEN["secp"], n, axis=0)), ptr(ks), 4, ptr(host), n))
            d = torch.from_numpy(host.view(np.int64)).cuda()
        else:
            d_gen = torch.from_numpy(np.repeat(GEN[group], n, axis=0).view(np.int64)).cuda()
            d_k = torch.from_numpy(ks.view(np.int64)).cuda()
            d = torch.empty((n, W[group]), dtype=torch.int64, device="cuda")
            zk.check(_fn(L, group, "mul_batch_dev")(_vp(d_gen), _vp(d_k), 4, _vp(d), n, None))
            torch.cuda.synchronize()
        _bases[group] = (d, M.ints_from_scalars(ks))
    return _bases[group]


def _free_handle(L):
    for (group, n), h in list(_handle.items()):
        _fn(L, group, "bases_free")(h)
    _handle.clear()


def _handle_for(L, group, n):
    """the resident set of the first n shared bases; one handle lives at a time (the cases are ordered by (group, n))"""
    if (group, n) not in _handle:
        _free_handle(L)
        d, _ = _base_set(L, group)
        h = ctypes.c_void_p()
        zk.check(_fn(L, group, "bases_from_device")(_vp(d), n, None, ctypes.byref(h)))
        assert _fn(L, group, "bases_len")(h) == n
        _handle[(group, n)] = h
    return _handle[(group, n)]


@pytest.fixture(scope="module", autouse=True)
def _release(L):
    yield
    _free_handle(L)
    _bases.clear()


def _expected(L, group, n, vec, key=None):
    """(1, W) python-integer point of one vector over the first n shared bases (cached under `key`)"""
    if key is not None and key in _want:
        return _want[key]
    kint = _base_set(L, group)[1][:n]
    tot = sum(k * s for k, s in zip(kint, M.ints_from_scalars(vec))) % M.ORDER[group]
    pt = _point(group, tot)
    if key is not None:
        _want[key] = pt
    return pt


def _pack(vectors, n, stride):
    """(k * stride, 4) uint64: vector v at row v * stride; the rows between the vectors hold a pattern no result may depend on"""
    k = len(vectors)
    buf = np.full((max(k * stride, 1), 4), 0xDEADBEEFCAFEF00D, np.uint64)
    for v, s in enumerate(vectors):
        buf[v * stride: v * stride + n] = s
    return buf


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _batch_dev(L, group, h, d_s, n, k, stride, partials=None):
    out = np.zeros((k, W[group]), np.uint64)
    zk.check(_fn(L, group, "msm_batch_dev")(h, _vp(d_s), n, k, stride, None, ptr(out), None if partials is None else _vp(partials)))
    return out


def _single_dev(L, group, h, d_vec, n):
    got = np.zeros((1, W[group]), np.uint64)
    zk.check(_fn(L, group, "msm_dev")(h, _vp(d_vec), n, None, ptr(got), None))
    return got


def _check_batch(L, group, n, vectors, stride, label, keys=None):
    """the batch over `vectors` == python integers == zkt_*_msm_dev of each vector alone"""
    k = len(vectors)
    h = _handle_for(L, group, n)
    d_s = _to_dev(_pack(vectors, n, stride))
    out = _batch_dev(L, group, h, d_s, n, k, stride)
    for v, vec in enumerate(vectors):
        key = None if keys is None else keys[v]
        want = _expected(L, group, n, vec, key)
        assert (out[v] == want[0]).all(), f"{group} {label}: out[{v}] of {k} differs from python integers"
        if key is None or key not in _single:
            one = _single_dev(L, group, h, _to_dev(vec), n)
            if key is not None:
                _single[key] = one
        else:
            one = _single[key]
        assert (out[v] == one[0]).all(), f"{group} {label}: out[{v}] of {k} differs from zkt_{group}_msm_dev of the vector alone"
    return out


def _is_inf(group, row):
    return (row == _point(group, 0)[0]).all()


_SIZES = [(g, n, k) for g in B.GROUPS for n in B.WIDTH_STEPS for k in B.BATCH_SIZES]


@pytest.mark.parametrize("group,n,k", _SIZES, ids=[f"{g}-n{n}-k{k}" for g, n, k in _SIZES])
def test_batch_widths_and_sizes(L, group, n, k):
    vectors = B.random_vectors(group, n, k)
    _check_batch(L, group, n, vectors, n, f"n={n}", keys=[(group, n, v) for v in range(k)])


@pytest.mark.parametrize("group", B.GROUPS)
def test_batch_of_an_empty_set_is_k_points_at_infinity(L, group):
    h = _handle_for(L, group, 0)
    d_s = _to_dev(np.zeros((4, 4), np.uint64))
    out = _batch_dev(L, group, h, d_s, 0, 3, 0)
    assert all(_is_inf(group, out[v]) for v in range(3))
    out = np.ones((3, W[group]), np.uint64)
    zk.check(_fn(L, group, "msm_batch_dev")(h, None, 0, 3, 5, None, ptr(out), None))          # no scalars to read: a null vector pointer is fine
    assert all(_is_inf(group, out[v]) for v in range(3))


@pytest.mark.parametrize("group", B.GROUPS)
def test_batch_mixed_vectors_with_a_padded_stride(L, group):
    n = B.MIXED_N
    vectors = B.mixed_vectors(group)
    out = _check_batch(L, group, n, vectors, n + B.MIXED_STRIDE_PAD, "mixed")
    assert _is_inf(group, out[1]) and not _is_inf(group, out[0])


_BOUND = [(g, n) for g in B.GROUPS for n in B.BOUNDARY_N]


@pytest.mark.parametrize("group,n", _BOUND, ids=[f"{g}-n{n}" for g, n in _BOUND])
def test_batch_bucket_set_boundary(L, group, n):
    """vector v only in the LAST bucket of its set, vector v + 1 only in the FIRST of the next — then the other way round"""
    for swapped in (False, True):
        vectors = B.boundary_vectors(n, group, swapped)
        keys = [(group, n, "first" if (v == 0) == swapped else "last") for v in range(2)]
        _check_batch(L, group, n, vectors, n, f"boundary n={n} swapped={swapped}", keys=keys)


@pytest.mark.parametrize("group", B.GROUPS)
def test_batch_partials_sum_to_the_points(L, group):
    import torch
    n, k = 2047, 5
    vectors = B.random_vectors(group, n, k)
    h = _handle_for(L, group, n)
    d_s = _to_dev(_pack(vectors, n, n))
    parts = torch.full((k * PW[group] + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = _batch_dev(L, group, h, d_s, n, k, n, partials=parts)
    assert (parts[k * PW[group]:].cpu().numpy() == 0x5A5A5A5A).all(), "the partials end after k * PARTIAL_WORDS words"
    for v in range(k):
        assert (out[v] == _expected(L, group, n, vectors[v], (group, n, v))[0]).all()
        got = np.zeros((1, W[group]), np.uint64)
        zk.check(_fn(L, group, "jac_sum_dev")(ctypes.c_void_p(parts.data_ptr() + 4 * v * PW[group]), 1, None, ptr(got)))
        assert (got[0] == out[v]).all(), f"{group}: partial {v} does not normalise to out[{v}]"
    # partials alone, and points alone through submit / collect
    parts2 = torch.zeros_like(parts)
    zk.check(_fn(L, group, "msm_batch_dev")(h, _vp(d_s), n, k, n, None, None, _vp(parts2)))
    got = np.zeros((1, W[group]), np.uint64)
    zk.check(_fn(L, group, "jac_sum_dev")(ctypes.c_void_p(parts2.data_ptr() + 4 * (k - 1) * PW[group]), 1, None, ptr(got)))
    assert (got[0] == out[k - 1]).all()
    zk.check(_fn(L, group, "msm_batch_submit")(h, _vp(d_s), n, k, n, None))
    out2 = np.zeros_like(out)
    zk.check(_fn(L, group, "msm_batch_collect")(h, ptr(out2), None))
    assert (out2 == out).all()


@pytest.mark.parametrize("group", B.GROUPS)
def test_batch_beside_slot_msms_on_one_handle(L, group):
    n, k = 2048, 3
    vectors = B.random_vectors(group, n, k)
    h = _handle_for(L, group, n)
    d_s = _to_dev(_pack(vectors, n, n))
    d_v = [_to_dev(vectors[v]) for v in (0, 1)]
    zk.check(_fn(L, group, "msm_batch_submit")(h, _vp(d_s), n, k, n, None))
    for slot in (0, 1):
        zk.check(_fn(L, group, "msm_submit")(h, _vp(d_v[slot]), n, None, slot))
    want = [_expected(L, group, n, vectors[v], (group, n, v)) for v in range(k)]
    for slot in (0, 1):
        got = np.zeros((1, W[group]), np.uint64)
        zk.check(_fn(L, group, "msm_collect")(h, slot, ptr(got), None))
        assert (got == want[slot]).all(), f"{group}: slot {slot} beside a batch"
    out = np.zeros((k, W[group]), np.uint64)
    zk.check(_fn(L, group, "msm_batch_collect")(h, ptr(out), None))
    for v in range(k):
        assert (out[v] == want[v][0]).all(), f"{group}: out[{v}] of a batch beside two slot MSMs"


@pytest.mark.parametrize("group", B.GROUPS)
def test_batch_reuse_and_steady_state(L, group):
    """k = 5, 2, 5, 5 with new scalars on one handle: every result right, and after the first batch with the largest k nothing is allocated"""
    import torch
    n = 2047
    h = _handle_for(L, group, n)
    runs = [(5, 80), (2, 90), (5, 100), (5, 110)]
    vecs = [B.random_vectors(group, n, k, seed) for k, seed in runs]
    d = [_to_dev(_pack(v, n, n)) for v in vecs]
    outs = [np.zeros((k, W[group]), np.uint64) for k, _ in runs]
    want = [[_expected(L, group, n, vec) for vec in v] for v in vecs]
    call = _fn(L, group, "msm_batch_dev")
    free = None
    for r, (k, _) in enumerate(runs):
        if r == 2:
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info()[0]                          # before the second k = 5 call
        zk.check(call(h, _vp(d[r]), n, k, n, None, ptr(outs[r]), None))
    assert torch.cuda.mem_get_info()[0] == free, "a batch allocated device memory after the first batch with the largest k"
    for r, (k, _) in enumerate(runs):
        for v in range(k):
            assert (outs[r][v] == want[r][v][0]).all(), f"{group}: run {r} (k = {k}) out[{v}]"


def _good_batch(L, group, h, n):
    vectors = B.random_vectors(group, n, 2)
    out = _batch_dev(L, group, h, _to_dev(_pack(vectors, n, n)), n, 2, n)
    for v in range(2):
        assert (out[v] == _expected(L, group, n, vectors[v], (group, n, v))[0]).all(), f"{group}: a good batch after a refused call"


@pytest.mark.parametrize("group", B.GROUPS)
def test_batch_shape_errors_leave_the_handle_usable(L, group):
    n = 1024
    h = _handle_for(L, group, n)
    d_s = _to_dev(_pack(B.random_vectors(group, n, 2), n, n))
    big = _to_dev(np.zeros((8, 4), np.uint64))                           # refused before any scalar is read
    out = np.zeros((40, W[group]), np.uint64)
    sub, col, dev = _fn(L, group, "msm_batch_submit"), _fn(L, group, "msm_batch_collect"), _fn(L, group, "msm_batch_dev")
    assert sub(None, _vp(d_s), n, 2, n, None) == SHAPE and col(None, ptr(out), None) == SHAPE and dev(None, _vp(d_s), n, 2, n, None, ptr(out), None) == SHAPE
    assert sub(h, _vp(d_s), n - 1, 2, n, None) == SHAPE and sub(h, _vp(d_s), n + 1, 2, n + 1, None) == SHAPE      # n != zkt_*_bases_len
    assert sub(h, _vp(big), n, 0, n, None) == SHAPE and sub(h, _vp(big), n, B.BATCH_MAX + 1, n, None) == SHAPE
    assert sub(h, _vp(d_s), n, 2, n - 1, None) == SHAPE                                                            # vec_stride < n
    assert dev(h, _vp(d_s), n, 2, n, None, None, None) == SHAPE                                                   # _dev needs an output
    assert col(h, ptr(out), None) == SHAPE                                                                         # nothing in flight — after all the refusals above
    zk.check(sub(h, _vp(d_s), n, 2, n, None))
    assert sub(h, _vp(d_s), n, 2, n, None) == SHAPE and dev(h, _vp(d_s), n, 2, n, None, ptr(out), None) == SHAPE   # a batch is in flight
    zk.check(col(h, None, None))                                                                                   # both outputs may be NULL in collect
    assert col(h, ptr(out), None) == SHAPE
    _good_batch(L, group, h, n)


def _generator_set(L, n):
    """a G1 set of n copies of the generator: the sum over it is (sum s_i) * G"""
    import torch
    d = torch.from_numpy(GEN["g1"].view(np.int64)).cuda().repeat(n, 1).contiguous()
    h = ctypes.c_void_p()
    zk.check(L.zkt_g1_bases_from_device(_vp(d), n, None, ctypes.byref(h)))
    return h


def test_batch_refuses_more_than_2p22_terms(L):
    """k * n > ZKT_MSM_BATCH_MAX_TERMS: n = 140000, k = 31 on G1 (k = 2 on the same handle is fine)"""
    _free_handle(L)
    n = 140000
    h = _generator_set(L, n)
    try:
        small = _to_dev(np.zeros((8, 4), np.uint64))
        out = np.zeros((31, G1W), np.uint64)
        assert L.zkt_g1_msm_batch_submit(h, _vp(small), n, 31, n, None) == SHAPE
        assert L.zkt_g1_msm_batch_dev(h, _vp(small), n, 31, n, None, ptr(out), None) == SHAPE
        assert L.zkt_g1_msm_batch_collect(h, ptr(out), None) == SHAPE
        s = np.zeros((2 * n, 4), np.uint64)
        s[:, 0] = np.random.Generator(np.random.PCG64(5)).integers(0, 2**64, size=2 * n, dtype=np.uint64)
        zk.check(L.zkt_g1_msm_batch_dev(h, _vp(_to_dev(s)), n, 2, n, None, ptr(out), None))
        for v in range(2):
            tot = sum(int(x) for x in s[v * n: (v + 1) * n, 0]) % M.R_ORDER
            assert (out[v] == _point("g1", tot)[0]).all(), f"a good batch of 2 x {n} terms after the refusal: out[{v}]"
    finally:
        L.zkt_g1_bases_free(h)


def test_batch_refuses_2p19_terms(L):
    """n = 2^19 on G1: every k is refused (zkt_g1_msm_submit is the form for that size); the handle still serves zkt_g1_msm_dev"""
    _free_handle(L)
    n = 1 << 19
    h = _generator_set(L, n)
    try:
        s = np.zeros((n, 4), np.uint64)
        s[:, 0] = np.random.Generator(np.random.PCG64(6)).integers(0, 2**64, size=n, dtype=np.uint64)
        d_s = _to_dev(s)
        out = np.zeros((2, G1W), np.uint64)
        for k in (1, 2):
            assert L.zkt_g1_msm_batch_submit(h, _vp(d_s), n, k, n, None) == SHAPE
            assert L.zkt_g1_msm_batch_dev(h, _vp(d_s), n, k, n, None, ptr(out), None) == SHAPE
        assert L.zkt_g1_msm_batch_collect(h, ptr(out), None) == SHAPE
        zk.check(L.zkt_g1_msm_dev(h, _vp(d_s), n, None, ptr(out), None))
        assert (out[0] == _point("g1", sum(int(x) for x in s[:, 0]) % M.R_ORDER)[0]).all()
    finally:
        L.zkt_g1_bases_free(h)


def test_batch_with_poisoned_workspaces():
    """This module again in a child process with ZKT_DEBUG_POISON=1: the batch workspace starts as 0xA5 bytes, so a kernel that reads a word nobody wrote
    (a slot of another vector, the partials of a bucket set that stayed empty, the task list behind the last set) fails instead of reading zeros."""
    if os.environ.get("ZKT_DEBUG_POISON"):
        pytest.skip("already inside the poisoned child")
    here = os.path.abspath(__file__)
    env = dict(os.environ, ZKT_DEBUG_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
