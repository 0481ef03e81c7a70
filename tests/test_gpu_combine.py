"""The multi-rank combine (k_jac_sum_to_affine behind zkt_{g1,g2,secp}_jac_sum_dev, zk-toolkit_amd/csrc/zkt_msm.hip) on exceptional partials, and the world-1
exchange of zkt_comm.cpp, against python integers.

The cases are tests/combine_model.py's: which lane meets which, and through which exit of jac_add, is proven on the CPU by tests/test_combine_model.py.  Partials
are opaque, so they come from the library: a resident set of four known multiples of the generator and zkt_*_msm_batch_dev (32 vectors a call, seven calls) leave a
pool of Jacobian partials whose discrete logarithms are the model's (scalar 0 is solved for, base 0 is the generator itself).  "P'" is the point of "P" from
another scalar vector — other bytes; "-P" comes from the negated scalars of "P"; infinity comes from an all-zero vector and from a resident set of no bases.
Every case is gathered from pool rows on the device into a fresh 0xA5 buffer one partial longer than the case; the expected point is
py_*_mul(generator, the model's sum)."""
import ctypes, functools, importlib, os, subprocess, sys
import numpy as np
import pytest
import combine_model as C
from zkt_testlib import (G1W, G2W, G1_GEN, G2_GEN, SECP_GEN, SplitMix64, py_g1_mul, py_g2_mul, py_secp_mul, g1_arr, g2_arr, secp_arr, to_abi_g2, ptr,
                         ints_to_arr)

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")

W = {"g1": G1W, "g2": G2W, "secp": 9}
PW = {"g1": zk.G1_PARTIAL_WORDS, "g2": zk.G2_PARTIAL_WORDS, "secp": zk.SECP_PARTIAL_WORDS}
GEN = {"g1": g1_arr([G1_GEN]), "g2": g2_arr([G2_GEN]), "secp": secp_arr([SECP_GEN])}
NB, BATCH, CALLS = 4, 32, 7                      # bases of the pool's resident set, vectors per zkt_*_msm_batch_dev, calls
POOL_ROWS = BATCH * CALLS                        # 224 batch partials; row 224 is the partial of the set of no bases
# pool row of every token of the model; the rows left over hold more all-zero vectors
ROW = {("g", i): i for i in range(C.GENERIC_N)}
ROW.update({"P": 200, "P'": 201, "-P": 202, "Q": 203, "inf0": 204, "infn": POOL_ROWS})
SPOT = (("g", 0), "P", "P'", "-P")               # affine outputs compared with python integers


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _fn(L, group, name):
    return getattr(L, f"zkt_{group}_{name}")


@functools.lru_cache(maxsize=None)
def _point(group, tot):
    """(1, W) ABI point tot * generator from python integers; tot None or 0 is infinity"""
    tot = tot or 0
    if group == "g1":
        return g1_arr([py_g1_mul(G1_GEN, tot)])
    if group == "secp":
        return secp_arr([py_secp_mul(SECP_GEN, tot)])
    (x1, x0), (y1, y0) = G2_GEN
    pt = py_g2_mul(((x0, x1), (y0, y1)), tot)
    return g2_arr([None if pt is None else to_abi_g2(pt)])


def _base_logs(group):
    """k_j of the pool's resident set: the generator, its double and two random multiples"""
    rng = SplitMix64(0xBA5E + C.GROUPS.index(group))
    return [1, 2, rng.below(C.ORDER[group] - 1) + 1, rng.below(C.ORDER[group] - 1) + 1]


def _make_bases(L, group, ks):
    """k_i * G on the device: zkt_*_mul_batch_dev (G1, G2) or the host-pointer batch (secp256k1 has no device form)"""
    import torch
    n = len(ks)
    ka = ints_to_arr(ks, 4)
    if group == "secp":
        host = np.zeros((n, 9), np.uint64)
        zk.check(L.zkt_secp_mul_batch(ptr(np.repeat(GEN["secp"], n, axis=0)), ptr(ka), 4, ptr(host), n))
        return torch.from_numpy(host.view(np.int64)).cuda()
    d_gen = torch.from_numpy(np.repeat(GEN[group], n, axis=0).view(np.int64)).cuda()
    d_k = torch.from_numpy(ka.view(np.int64)).cuda()
    d_out = torch.empty((n, W[group]), dtype=torch.int64, device="cuda")
    zk.check(_fn(L, group, "mul_batch_dev")(_vp(d_gen), _vp(d_k), 4, _vp(d_out), n, None))
    torch.cuda.synchronize()
    return d_out


def _vector(group, ks, c, rng):
    """four scalars below the order with sum k_j s_j = c mod order: s_1 .. s_3 random, s_0 solved for (k_0 = 1)"""
    order = C.ORDER[group]
    s = [0] + [rng.below(order) for _ in range(NB - 1)]
    s[0] = (c - sum(k * x for k, x in zip(ks[1:], s[1:]))) % order
    assert sum(k * x for k, x in zip(ks, s)) % order == c % order
    return s


def _pool_vectors(group):
    """POOL_ROWS scalar vectors (python ints) in pool-row order"""
    order, ks, lg, rng = C.ORDER[group], _base_logs(group), C.logs(group), SplitMix64(0x5CA1 + C.GROUPS.index(group))
    vec = [[0] * NB for _ in range(POOL_ROWS)]
    for i in range(C.GENERIC_N):
        vec[ROW[("g", i)]] = _vector(group, ks, lg[("g", i)], rng)
    for tok in ("P", "P'", "Q"):
        vec[ROW[tok]] = _vector(group, ks, lg[tok], rng)
    vec[ROW["-P"]] = [(order - x) % order for x in vec[ROW["P"]]]
    assert vec[ROW["P"]] != vec[ROW["P'"]] and sum(k * x for k, x in zip(ks, vec[ROW["-P"]])) % order == lg["-P"]
    return vec


_pools = {}


def _pool(L, group):
    """(device tensor (POOL_ROWS + 1, PW) int32 of Jacobian partials, host array (POOL_ROWS + 1, W) of their affine points), built once per group"""
    import torch
    if group not in _pools:
        ks, vec = _base_logs(group), _pool_vectors(group)
        d_bases = _make_bases(L, group, ks)
        pool = torch.zeros((POOL_ROWS + 1, PW[group]), dtype=torch.int32, device="cuda")
        aff = np.zeros((POOL_ROWS + 1, W[group]), np.uint64)
        h = ctypes.c_void_p()
        zk.check(_fn(L, group, "bases_from_device")(_vp(d_bases), NB, None, ctypes.byref(h)))
        try:
            for call in range(CALLS):
                rows = slice(call * BATCH, (call + 1) * BATCH)
                d_s = torch.from_numpy(ints_to_arr([x for v in vec[rows] for x in v], 4).view(np.int64)).cuda()
                zk.check(_fn(L, group, "msm_batch_dev")(h, _vp(d_s), NB, BATCH, NB, None, aff[rows].ctypes.data, _vp(pool[call * BATCH])))
        finally:
            _fn(L, group, "bases_free")(h)
        h0 = ctypes.c_void_p()
        zk.check(_fn(L, group, "bases_upload")(None, 0, ctypes.byref(h0)))          # the resident set of an empty shard
        try:
            assert _fn(L, group, "bases_len")(h0) == 0
            zk.check(_fn(L, group, "msm_dev")(h0, None, ctypes.c_size_t(0), None, ctypes.c_void_p(aff[POOL_ROWS:].ctypes.data), _vp(pool[POOL_ROWS])))
        finally:
            _fn(L, group, "bases_free")(h0)
        torch.cuda.synchronize()
        _pools[group] = (pool, aff)
    return _pools[group]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _pools.clear()


def _sum_case(L, group, case, stream=None):
    """the case's partials gathered into a fresh poisoned buffer with one guard partial behind them -> the (1, W) point zkt_*_jac_sum_dev returns"""
    import torch
    pool, _ = _pool(L, group)
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        idx = torch.tensor([ROW[t] for t in case.tokens], dtype=torch.int64, device="cuda")
        buf = torch.full(((case.count + 1) * PW[group] * 4,), 0xA5, dtype=torch.uint8, device="cuda")
        buf.view(torch.int32).view(case.count + 1, PW[group])[: case.count] = pool[idx]
    if stream is None:
        torch.cuda.synchronize()
    got = np.full((1, W[group]), 0x5A5A5A5A5A5A5A5A, np.uint64)
    zk.check(_fn(L, group, "jac_sum_dev")(_vp(buf), ctypes.c_size_t(case.count), None if stream is None else ctypes.c_void_p(stream.cuda_stream), ptr(got)))
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32).view(case.count + 1, PW[group])[case.count] == torch.tensor(0xA5A5A5A5 - (1 << 32), dtype=torch.int32)).all())
    return got


@pytest.mark.parametrize("group", C.GROUPS)
def test_the_pool_holds_the_models_partials(L, group):
    """four affine outputs against python integers, both infinities, P and P' the same point in other bytes, and (G1) the zero padding word of every coordinate"""
    pool, aff = _pool(L, group)
    lg = C.logs(group)
    for tok in SPOT:
        assert (aff[ROW[tok]] == _point(group, lg[tok])[0]).all(), tok
    for tok in C.INF_TOKENS:
        assert (aff[ROW[tok]] == _point(group, None)[0]).all(), tok
    words = pool.cpu().numpy().view(np.uint32)
    assert (aff[ROW["P"]] == aff[ROW["P'"]]).all()
    # the cross-multiplied equality of jac_add needs two representations of one point: if these ever coincide the partials got normalised and P' needs another construction
    assert (words[ROW["P"]] != words[ROW["P'"]]).any(), "P and P' have the same bytes"
    cw = PW[group] // 3
    assert not words[ROW["inf0"], 2 * cw:].any() and not words[ROW["infn"], 2 * cw:].any(), "Z of a partial at infinity"
    if group == "g1":
        assert (words[:, [13, 27, 41]] == 0).all(), np.argwhere(words[:, [13, 27, 41]] != 0)[:8]


_CASES = [(g, c.name) for g in C.GROUPS for c in C.CASES]


@pytest.mark.parametrize("group,name", _CASES, ids=[f"{g}-{n}" for g, n in _CASES])
def test_jac_sum_case(L, group, name):
    case = C.CASE[name]
    assert not C.check_claim(case, group)
    got = _sum_case(L, group, case)
    assert (got == _point(group, case.run(group).total)).all(), f"{group} {name}: zkt_{group}_jac_sum_dev differs from python integers"


@pytest.mark.parametrize("group", C.GROUPS)
def test_jac_sum_on_a_caller_stream(L, group):
    """the gather is queued on the caller's stream and not waited for: the call orders its kernel behind it"""
    import torch
    case = C.CASE["distinct-129"]
    got = _sum_case(L, group, case, stream=torch.cuda.Stream())
    assert (got == _point(group, case.run(group).total)).all()


@pytest.mark.parametrize("group", C.GROUPS)
def test_jac_sum_refusals_leave_the_output_alone(L, group):
    assert C.REJECTS == ("count0", "null_partials", "null_out")
    pool, _ = _pool(L, group)
    fn = _fn(L, group, "jac_sum_dev")
    got = np.full((1, W[group]), 0x5A5A5A5A5A5A5A5A, np.uint64)
    assert fn(_vp(pool), ctypes.c_size_t(0), None, ptr(got)) == zk.ZKT_ERR_SHAPE
    assert fn(None, ctypes.c_size_t(2), None, ptr(got)) == zk.ZKT_ERR_SHAPE
    assert fn(_vp(pool), ctypes.c_size_t(2), None, None) == zk.ZKT_ERR_SHAPE
    assert (got == 0x5A5A5A5A5A5A5A5A).all()
    zk.check(fn(_vp(pool), ctypes.c_size_t(2), None, ptr(got)))                   # and the next call is served
    lg = C.logs(group)
    assert (got == _point(group, (lg[("g", 0)] + lg[("g", 1)]) % C.ORDER[group])).all()


# ---- the world-1 exchange ---------------------------------------------------------------------------------------------------------------
N_TERMS = 65


def test_world1_exchange(L):
    """zkt_comm_init(0, 1, NULL), then zkt_*_msm_sharded and submit + zkt_*_msm_sharded_collect on three slots: a resident set of no bases (n_local = 0), an
    all-zero scalar vector and 65 terms.  One rank: the combine sums one partial, so each result is the python-integer point of the rank's own MSM."""
    import torch
    zk.check(L.zkt_comm_init(0, 1, None))
    try:
        assert L.zkt_comm_rank() == 0 and L.zkt_comm_world() == 1
        for group in C.GROUPS:
            order, rng = C.ORDER[group], SplitMix64(0x0E1 + C.GROUPS.index(group))
            ks = [rng.below(order - 1) + 1 for _ in range(N_TERMS)]
            vecs = [[rng.below(order) for _ in range(N_TERMS)] for _ in range(3)]
            d_bases = _make_bases(L, group, ks)
            zero = torch.zeros((N_TERMS, 4), dtype=torch.int64, device="cuda")
            d_vecs = [torch.from_numpy(ints_to_arr(v, 4).view(np.int64)).cuda() for v in vecs]
            tots = [sum(k * s for k, s in zip(ks, v)) % order for v in vecs]
            h, h0 = ctypes.c_void_p(), ctypes.c_void_p()
            zk.check(_fn(L, group, "bases_from_device")(_vp(d_bases), N_TERMS, None, ctypes.byref(h)))
            zk.check(_fn(L, group, "bases_upload")(None, 0, ctypes.byref(h0)))
            try:
                for what, hh, n, scal, want in (("no bases", h0, 0, [None] * 3, [None] * 3), ("zero scalars", h, N_TERMS, [_vp(zero)] * 3, [None] * 3),
                                                ("65 terms", h, N_TERMS, [_vp(d) for d in d_vecs], tots)):
                    got = np.full((1, W[group]), 0x5A5A5A5A5A5A5A5A, np.uint64)
                    zk.check(_fn(L, group, "msm_sharded")(hh, scal[0], ctypes.c_size_t(n), None, ptr(got)))
                    assert (got == _point(group, want[0])).all(), f"{group} {what}: zkt_{group}_msm_sharded"
                    for slot in range(3):
                        zk.check(_fn(L, group, "msm_submit")(hh, scal[slot], n, None, slot))
                    for slot in range(3):
                        got = np.full((1, W[group]), 0x5A5A5A5A5A5A5A5A, np.uint64)
                        zk.check(_fn(L, group, "msm_sharded_collect")(hh, slot, ptr(got)))
                        assert (got == _point(group, want[slot])).all(), f"{group} {what}: slot {slot} through zkt_{group}_msm_sharded_collect"
            finally:
                _fn(L, group, "bases_free")(h)
                _fn(L, group, "bases_free")(h0)
    finally:
        L.zkt_comm_finalize()


def test_world1_exchange_as_a_local_copy():
    """test_world1_exchange again in a child process with ZKT_COMM_LOCAL_WORLD1=1: no RCCL communicator, the exchange is a device-to-device copy — the path of a
    single-GPU consumer without RCCL"""
    here = os.path.abspath(__file__)
    env = dict(os.environ, ZKT_COMM_LOCAL_WORLD1="1")
    r = subprocess.run([sys.executable, "-m", "pytest", here + "::test_world1_exchange", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout
