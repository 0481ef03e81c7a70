"""GPU: every batched primitive of include/zkt.h rows a1-a8, a16, a18 on the case lists of tests/prim_cases.py, bit-exact against python integers, status codes and
zkt_last_error_index() included.  The device build is its own compilation of the kernel headers (inline-assembly multiply-add, called multiplies, per-object flags):
tests/test_prim_cases.py vouches for the host build of the same lists, this file for the device.  Output arrays are pre-filled, so an element a kernel skipped shows."""
import ctypes, importlib
import numpy as np
import pytest
import prim_cases as pc
from prim_cases import FIELDS, GROUPS, pack, unpack, pack_tower, unpack_tower, pack_points, unpack_points, check
from zkt_testlib import ZKT_OK, ZKT_ERR_INV_ZERO, ZKT_ERR_SHAPE, R, SECP_N, SplitMix64, ptr

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
PATTERN = 0xA5A5A5A5A5A5A5A5
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def filled(shape):
    return np.full(shape, PATTERN, dtype=np.uint64)


def _idx(L, rc):
    return L.zkt_last_error_index() if rc == ZKT_ERR_INV_ZERO else None


# ---- runners: one batch through the C ABI -> (status, error index, outputs) ----------------------------------------------------------------------
def field_gpu(L, b):
    pre, op, w = b["pre"], b["op"], FIELDS[b["pre"]]["w"]
    a = pack(b["a"], w); n = len(b["a"])
    if op in ("add", "sub", "mul"):
        o = filled(a.shape); rc = getattr(L, "zkt_%s_%s_batch" % (pre, op))(ptr(a), ptr(pack(b["b"], w)), ptr(o), sz(n))
        return rc, _idx(L, rc), unpack(o)
    if op in ("sqr", "cube", "neg", "inv"):
        o = filled(a.shape); rc = getattr(L, "zkt_%s_%s_batch" % (pre, op))(ptr(a), ptr(o), sz(n))
        return rc, _idx(L, rc), unpack(o)
    if op == "pow":
        e = pack([b["k"]] if b["shared"] else b["b"], b["exp_limbs"]); o = filled(a.shape)
        return getattr(L, "zkt_%s_pow_batch" % pre)(ptr(a), ptr(e), b["exp_limbs"], b["shared"], ptr(o), n), None, unpack(o)
    if op == "scale":
        o = filled(a.shape)
        return getattr(L, "zkt_%s_scale_batch" % pre)(ptr(a), ptr(pack([b["k"]], w)), ptr(o), sz(n)), None, unpack(o)
    if op == "sum":
        o = filled((1, w))
        return getattr(L, "zkt_%s_sum" % pre)(ptr(a), sz(n), ptr(o)), None, unpack(o)[0]
    o = filled((b["n"], w))
    return getattr(L, "zkt_%s_%s" % (pre, op))(ptr(a), b["n"], ptr(o)), None, unpack(o)


def tower_gpu(L, b):
    d, op = b["deg"], b["op"]
    a = pack_tower(b["a"]); o = filled(a.shape); n = len(a)
    fn = getattr(L, "zkt_fq%d_%s_batch" % (d, op))
    rc = fn(ptr(a), ptr(pack_tower(b["b"])), ptr(o), sz(n)) if op in ("add", "sub", "mul") else fn(ptr(a), ptr(o), sz(n))
    return rc, _idx(L, rc), unpack_tower(o, d)


def fq12_pow_gpu(L, b):
    a = pack_tower(b["a"]); o = filled(a.shape)
    e = np.array([(b["e"] >> (32 * i)) & 0xFFFFFFFF for i in range(b["nl"])], dtype=np.uint32)
    rc = L.zkt_fq12_pow_batch(ptr(a), e.ctypes.data_as(ctypes.c_void_p), sz(b["nl"]), ptr(o), sz(len(a)))
    return rc, None, unpack_tower(o, 12)


def group_gpu(L, b):
    grp, op = b["grp"], b["op"]; G = GROUPS[grp]
    a = pack_points(grp, b["pts"]); n = len(a)
    if op == "add":
        o = filled(a.shape)
        return getattr(L, "zkt_%s_add_batch" % grp)(ptr(a), ptr(pack_points(grp, b["pts_b"])), ptr(o), sz(n)), None, unpack_points(grp, o)
    if op == "neg":
        o = filled(a.shape)
        return getattr(L, "zkt_%s_neg_batch" % grp)(ptr(a), ptr(o), sz(n)), None, unpack_points(grp, o)
    if op in ("mul", "scale"):
        o = filled(a.shape); Lw = b["L"]
        ks = pack(b["ks"], max(1, min(Lw, 6)))
        rc = getattr(L, "zkt_%s_%s_batch" % (grp, op))(ptr(a), ptr(ks), Lw, ptr(o), sz(n))
        if rc != ZKT_OK:
            assert (o == PATTERN).all(), "a refused call wrote to its output"
            return rc, None, None
        return rc, None, unpack_points(grp, o)
    if op == "sum":
        o = filled((1, G["words"]))
        return getattr(L, "zkt_%s_sum" % grp)(ptr(a) if n else None, sz(n), ptr(o)), None, unpack_points(grp, o)[0]
    o = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    rc = getattr(L, "zkt_%s_%s_batch" % (grp, op))(ptr(a), o.ctypes.data_as(ctypes.c_void_p), n)
    return rc, None, [int(v) for v in o]


# ---- fields, tower, groups on the case lists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(FIELDS))
def test_fields(L, pre):
    for b in pc.field_batches(pre): check(b, *field_gpu(L, b), who="gpu")
    a = pack([1, 2], FIELDS[pre]["w"]); o = filled(a.shape)                    # empty batches: nothing written; an empty sum / scale is the reference's assert
    for op in ("add", "mul"): assert getattr(L, "zkt_%s_%s_batch" % (pre, op))(ptr(a), ptr(a), ptr(o), sz(0)) == ZKT_OK
    assert getattr(L, "zkt_%s_inv_batch" % pre)(ptr(a), ptr(o), sz(0)) == ZKT_OK
    assert getattr(L, "zkt_%s_sum" % pre)(ptr(a), sz(0), ptr(o)) == ZKT_ERR_SHAPE and getattr(L, "zkt_%s_scale_batch" % pre)(ptr(a), ptr(a), ptr(o), sz(0)) == ZKT_ERR_SHAPE
    assert getattr(L, "zkt_%s_pow_batch" % pre)(ptr(a), ptr(a), 0, 0, ptr(o), 2) == ZKT_ERR_SHAPE and getattr(L, "zkt_%s_pow_batch" % pre)(ptr(a), ptr(a), 65, 0, ptr(o), 2) == ZKT_ERR_SHAPE
    assert (o == PATTERN).all()


@pytest.mark.parametrize("deg", [2, 6, 12])
def test_tower(L, deg):
    for b in pc.tower_batches(deg): check(b, *tower_gpu(L, b), who="gpu")


def test_fq12_pow(L):
    for b in pc.fq12_pow_batches(): check(b, *fq12_pow_gpu(L, b), who="gpu")
    a = pack_tower([(1,) * 12]); o = filled(a.shape); e = np.array([3], dtype=np.uint32)
    assert L.zkt_fq12_pow_batch(ptr(a), e.ctypes.data_as(ctypes.c_void_p), sz(0), ptr(o), sz(1)) == ZKT_ERR_SHAPE and L.zkt_fq12_pow_batch(ptr(a), None, sz(1), ptr(o), sz(1)) == ZKT_ERR_SHAPE
    assert (o == PATTERN).all()


@pytest.mark.parametrize("grp", list(GROUPS))
def test_groups(L, grp):
    for b in pc.group_add_batches(grp) + pc.group_unary_batches(grp) + pc.group_mul_batches(grp) + pc.group_mul_geometry_batches(grp) + pc.group_sum_batches(grp):
        check(b, *group_gpu(L, b), who="gpu")


def test_generator_comb(L):
    """zkt_bls_public_keys_batch: the generator's comb table on nibble patterns (zero nibbles skipped, all-F, one nibble per position, k >= r used as it is), n across a block edge"""
    cs = pc.comb_scalars(); F = GROUPS["g1"]["F"]
    assert len(cs) > pc.GROUP_BLOCK
    want = [pc.aff_mul(F, GROUPS["g1"]["gen"], k) for _, k in cs]
    o = filled((len(cs), 13))
    rc = L.zkt_bls_public_keys_batch(ptr(pack([k for _, k in cs], 4)), len(cs), ptr(o))
    check(dict(kind="comb", grp="g1", rc=ZKT_OK, want=want, labels=[l for l, _ in cs]), rc, None, unpack_points("g1", o), who="gpu")


@pytest.mark.parametrize("grp", list(GROUPS))
def test_generators(L, grp):
    """row a16: zkt_*_generator returns the group's standard generator, canonical, flag and padding zero - the constant the case lists and the comb table start from"""
    o = filled((1, GROUPS[grp]["words"]))
    getattr(L, "zkt_%s_generator" % grp)(ptr(o))
    assert (o == pack_points(grp, [pc.ipt(GROUPS[grp]["gen"])])).all()
    assert pc.on_curve(grp, GROUPS[grp]["gen"]) == 1


# ---- point sums above one grid: 4,096 points is the last size with one lane per point ----------------------------------------------------------------
@pytest.mark.parametrize("grp", list(GROUPS))
def test_point_sums_above_one_grid(L, grp):
    """bases s_i G from the library's own scalar multiplication (spot-checked against python), sums of 4,095 / 4,096 / 4,097 / 8,193 of them against ONE python
    multiplication (sum s_i mod order) G; every base is different, so a point skipped, or added twice, changes the sum"""
    G = GROUPS[grp]; F = G["F"]; W = G["words"]
    sizes = pc.sum_sizes(pc.POINT_SUM_EDGE); n = max(sizes)
    rng = SplitMix64(0x5115 + G["id"])
    ss = [rng.next() | 1 for _ in range(n)]
    assert len(set(ss)) == n
    bases = filled((n, W))
    if grp == "g1":
        assert L.zkt_bls_public_keys_batch(ptr(pack(ss, 4)), n, ptr(bases)) == ZKT_OK
    else:
        gen = np.repeat(pack_points(grp, [pc.ipt(G["gen"])]), n, axis=0)
        assert getattr(L, "zkt_%s_mul_batch" % grp)(ptr(gen), ptr(pack(ss, 1)), 1, ptr(bases), sz(n)) == ZKT_OK
    for i in (0, 4095, 4096, n - 1):
        assert unpack_points(grp, bases[i:i + 1])[0] == pc.aff_mul(F, G["gen"], ss[i]), i
    for m in sizes:
        o = filled((1, W))
        rc = getattr(L, "zkt_%s_sum" % grp)(ptr(bases), sz(m), ptr(o))
        check(dict(kind="group", grp=grp, op="sum", label="n=%d" % m, rc=ZKT_OK, want=pc.aff_mul(F, G["gen"], sum(ss[:m]) % G["order"])), rc, None, unpack_points(grp, o)[0], who="gpu")
    # the same above the edge with the sum infinity: the last point is minus the sum of the others
    m = pc.POINT_SUM_EDGE + 1
    last = pack_points(grp, [pc.ipt(pc.aff_mul(F, G["gen"], (-sum(ss[:m - 1])) % G["order"]))])
    pts = np.concatenate([bases[:m - 1], last]); o = filled((1, W))
    assert getattr(L, "zkt_%s_sum" % grp)(ptr(pts), sz(m), ptr(o)) == ZKT_OK and unpack_points(grp, o)[0] is None


# ---- device-pointer entry points on a caller's stream ---------------------------------------------------------------------------------------------
def _dev(t):
    return ctypes.c_void_p(t.data_ptr())


def test_dev_entry_points_on_a_caller_stream(L):
    """zkt_fq_mul_batch_dev / zkt_g1_mul_batch_dev / zkt_g2_mul_batch_dev on a non-default stream whose inputs were produced on that stream just before; the output
    buffer is one row longer than n and pre-filled: rows < n equal python (hence the host-pointer call, checked by the tests above), the guard row is untouched"""
    import torch
    st = torch.cuda.Stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    def roundtrip(arr):                                   # produce the input ON the stream: upload, then a device-side copy
        with torch.cuda.stream(st):
            return torch.from_numpy(arr.view(np.int64)).cuda(non_blocking=True).clone()
    def guard(rows, width):
        with torch.cuda.stream(st):
            return torch.full((rows, width), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")      # 0xA5A5... as int64
    # Fq products: the labelled pairs of the field cases, n across a block edge
    core, _ = pc.field_pairs("fq")
    cs = pc.layout(core, pc.field_filler("fq", 600, 3), 2 * pc.FIELD_BLOCK + 1, pc.FIELD_BLOCK)
    n = len(cs); p = FIELDS["fq"]["p"]
    a, b = pack([c[1] for c in cs], 6), pack([c[2] for c in cs], 6)
    da, db, do = roundtrip(a), roundtrip(b), guard(n + 1, 6)
    assert L.zkt_fq_mul_batch_dev(_dev(da), _dev(db), _dev(do), sz(n), sp) == ZKT_OK
    st.synchronize()
    got = do.cpu().numpy().view(np.uint64)
    check(dict(kind="field", pre="fq", op="mul_dev", rc=ZKT_OK, labels=[c[0] for c in cs], want=[x * y % p for _, x, y in cs]), 0, None, unpack(got[:n]), who="gpu")
    assert (got[n] == PATTERN).all(), "guard row written"
    host = filled(a.shape)
    assert L.zkt_fq_mul_batch(ptr(a), ptr(b), ptr(host), sz(n)) == ZKT_OK and (host == got[:n]).all()
    assert L.zkt_fq_mul_batch_dev(_dev(da), _dev(db), _dev(do), sz(0), sp) == ZKT_OK                     # n = 0: a no-op
    st.synchronize()
    assert (do.cpu().numpy().view(np.uint64) == got).all()
    # point products, scalar_limbs 1..6 and the refused widths
    for grp, fn in (("g1", L.zkt_g1_mul_batch_dev), ("g2", L.zkt_g2_mul_batch_dev)):
        G = GROUPS[grp]; W = G["words"]
        for b_ in [x for x in pc.group_mul_batches(grp) if x["op"] == "mul" and x["L"] in (1, 4, 6)] + pc.group_mul_geometry_batches(grp)[3:4]:
            pts = pack_points(grp, b_["pts"]); n = len(pts)
            dp, dk, do = roundtrip(pts), roundtrip(pack(b_["ks"], b_["L"])), guard(n + 1, W)
            assert fn(_dev(dp), _dev(dk), b_["L"], _dev(do), sz(n), sp) == ZKT_OK
            st.synchronize()
            got = do.cpu().numpy().view(np.uint64)
            check(b_, 0, None, unpack_points(grp, got[:n]), who="gpu dev")
            assert (got[n] == PATTERN).all(), "guard row written"
            host = filled(pts.shape)
            assert getattr(L, "zkt_%s_mul_batch" % grp)(ptr(pts), ptr(pack(b_["ks"], b_["L"])), b_["L"], ptr(host), sz(n)) == ZKT_OK and (host == got[:n]).all()
        for bad in (0, 7):
            assert fn(_dev(dp), _dev(dk), bad, _dev(do), sz(1), sp) == ZKT_ERR_SHAPE
        assert fn(_dev(dp), _dev(dk), 4, _dev(do), sz(0), sp) == ZKT_OK
        st.synchronize()
        assert (do.cpu().numpy().view(np.uint64) == got).all()


def test_gt_eq(L):
    pv = pc.pairing_value()
    a = pack_tower([pv]); b = a.copy()
    assert L.zkt_gt_eq(ptr(a), ptr(b)) == 1
    b[0, 71] ^= np.uint64(1 << 60)                                             # differs in the last limb only
    assert L.zkt_gt_eq(ptr(a), ptr(b)) == 0
    b = a.copy(); b[0, 0] ^= np.uint64(1)                                       # ... in the first
    assert L.zkt_gt_eq(ptr(a), ptr(b)) == 0
    assert L.zkt_gt_eq(None, ptr(b)) == -ZKT_ERR_SHAPE and L.zkt_gt_eq(ptr(a), None) == -ZKT_ERR_SHAPE and L.zkt_gt_eq(None, None) == -ZKT_ERR_SHAPE
