"""CPU side of tests/prim_cases.py: the census of its case lists (every class populated or proven empty), the batch-geometry constants against the source text,
and the case lists through the oracle and through both host builds of the kernel headers (csrc/hostcheck.cpp), bit-exact against python integers.
The device build is a different compilation of the same headers: tests/test_gpu_primitives.py runs the same lists there."""
import ctypes, os, re
import numpy as np
import pytest
import prim_cases as pc
from prim_cases import FIELDS, GROUPS, pack, unpack, pack_tower, unpack_tower, pack_points, unpack_points, check
from zkt_testlib import ROOT, ZKT_OK, ZKT_ERR_INV_ZERO, oracle, ptr
from test_hostcheck import H, p32          # noqa: F401  (the fixture: the plain and the Karatsuba host build)

O = oracle()
_long = ctypes.c_long
GRP_O = {"g1": "g1", "g2": "g2", "secp": "secp"}


# ---- census and geometry --------------------------------------------------------------------------------------------------------------------------
def test_geometry_constants_match_the_source():
    c = pc.source_constants()
    assert c == {"FIELD_BLOCK": pc.FIELD_BLOCK, "TOWER_BLOCK": pc.TOWER_BLOCK, "GROUP_BLOCK": pc.GROUP_BLOCK, "SUM_MAX_BLOCKS": pc.SUM_MAX_BLOCKS, "SUM_BLOCKS": pc.SUM_BLOCKS}
    assert pc.sum_sizes(pc.FIELD_SUM_EDGE) == [65535, 65536, 65537, 131073] and pc.sum_sizes(pc.POINT_SUM_EDGE) == [4095, 4096, 4097, 8193]
    assert pc.elementwise_sizes(pc.FIELD_BLOCK, 200)[:5] == [1, 255, 256, 257, 513] and pc.elementwise_sizes(64, 100)[:5] == [1, 63, 64, 65, 129]


@pytest.mark.parametrize("pre", list(FIELDS))
def test_field_census(pre):
    """every class of the field's conditional subtractions is reached by a labelled case, or listed as unreachable with the reason (and then really empty)"""
    batches = pc.field_batches(pre)
    c = pc.field_census(pre, batches)
    lines = []
    for k in pc.field_classes(pre):
        why = pc.UNREACHABLE.get((pre, k))
        lines.append("%-34s %8d  %s" % (k, c[k], "unreachable because " + why if why else ""))
        assert (c[k] == 0) if why else (c[k] > 0), (pre, k, c[k])
    assert c["inverse of zero -> error"] >= 5
    print("\n".join(["census " + pre] + lines))
    # the crafted classes come from the crafted families, not from luck: without them the narrow window stays empty for secp256k1's fields
    if pre in ("sp", "sn"):
        core, cross = pc.field_pairs(pre)
        assert sum(1 for l, a, b in core if l.startswith("product") and "t1in[p,2^256)" in pc.product_classes(pre, a, b)) >= 2
        assert sum(1 for l, a, b in core if l.startswith("sum=") and FIELDS[pre]["p"] <= a + b < 1 << 256) >= 3
    # every element of an elementwise batch differs from the others; the long sum's terms too
    for b in batches:
        if b["op"] in ("add", "sub", "mul"): assert len(set(zip(b["a"], b["b"]))) == len(b["a"]), (b["op"], len(b["a"]))
        if b["op"] == "sum" and b["labels"] is None: assert len(set(b["a"])) == len(b["a"])
    sizes = {len(b["a"]) for b in batches if b["op"] == "sum"}
    assert set(pc.sum_sizes(pc.FIELD_SUM_EDGE)) <= sizes
    for op in ("add", "sub", "mul", "sqr", "cube", "neg", "inv"):
        assert set(pc.elementwise_sizes(pc.FIELD_BLOCK, 200)[:5]) <= {len(b["a"]) for b in batches if b["op"] == op and b["rc"] == ZKT_OK}, op
    big_n = pc.elementwise_sizes(pc.FIELD_BLOCK, 200)[5]
    assert big_n == 200 * pc.FIELD_BLOCK + 3
    for op in ("add", "sub", "mul", "sqr", "cube", "neg", "inv", "scale", "pow", "pow_seq", "repeat"):         # one size of a few hundred blocks for EVERY elementwise entry point
        ok = [b for b in batches if b["op"] == op and b["rc"] == ZKT_OK and not b.get("shared")]
        m = max(ok, key=lambda b: b.get("n", len(b["a"])))
        assert m.get("n", len(m["a"])) >= 100 * pc.FIELD_BLOCK, (op, m.get("n", len(m["a"])))
        if op in ("sqr", "cube", "neg", "inv", "scale"): assert len(m["a"]) == big_n and len(set(m["a"])) == big_n, op      # pairwise different
        if op == "pow": assert len(m["a"]) == big_n and len(set(zip(m["a"], m["b"]))) == big_n
    assert {b["exp_limbs"] for b in batches if b["op"] == "pow"} == {1, 2, 3, 4, 5, 6, 16} and {b["shared"] for b in batches if b["op"] == "pow"} == {0, 1}


@pytest.mark.parametrize("grp", list(GROUPS))
def test_group_census(grp):
    c = pc.group_census(grp)
    lines = ["census " + grp]
    for arm in pc.ADD_ARMS:
        lines.append("%-40s %4d" % (arm, c[arm])); assert c[arm] > 0, arm
    for L in range(1, 7):
        for k in ("carry out of the top limb", "no carry out"):
            lines.append("%-40s %4d" % ("L=%d: %s" % (L, k), c["L=%d: %s" % (L, k)])); assert c["L=%d: %s" % (L, k)] > 0, (L, k)
    print("\n".join(lines))
    # honest products are ((k s) mod order) G: the model's LSB-first loop against one more multiplication
    G = GROUPS[grp]; F = G["F"]; H_ = pc.group_points(grp)["honest"]
    k = sorted(H_)[5]
    for _, s in pc.scalar_list(grp, 6)[4:8]:
        assert pc.aff_mul(F, H_[k], s) == pc.aff_mul(F, G["gen"], k * s % G["order"])
    assert all(pc.on_curve(grp, p) == 1 and pc.in_subgroup(grp, p) == 1 for p in list(H_.values())[:3])
    assert all(pc.on_curve(grp, p) == 0 for p in pc.group_points(grp)["off"] + pc.group_points(grp)["singular"])
    assert all(pc.on_curve(grp, p) == 1 and pc.in_subgroup(grp, p) == 0 for _, p in pc.group_points(grp)["outside"])
    for b in pc.group_add_batches(grp):
        assert len(set(zip(b["pts"], b["pts_b"]))) == len(b["pts"])
    assert set(pc.elementwise_sizes(64, 100)) <= {len(b["pts"]) for b in pc.group_add_batches(grp)}


def test_tower_case_families():
    for d in (2, 6, 12):
        labels = " | ".join(l for l, _ in pc.tower_elements(d))
        for fam in ("every coefficient p-1", "alternating", "only coefficient %d" % (d - 1), "in Fq", "zero coefficients", "not reduced"):
            assert fam in labels, (d, fam)
        bs = pc.tower_batches(d)
        assert sum(1 for b in bs if b["rc"] == ZKT_ERR_INV_ZERO) == 5
        zero = (0,) * d
        for op in ("add", "sub", "mul"):
            assert sum(w == zero for b in bs if b["op"] == op for w in b["want"]) >= 10, (d, op)        # results whose every coefficient is zero
        one = (0,) * (d - 1) + (1,)
        assert sum(w == one for b in bs if b["op"] == "mul" for w in b["want"]) >= 10                    # a * a^-1: d - 1 zero coefficients
        for op in ("add", "sub", "mul", "neg", "inv") + (("reduce",) if d < 12 else ()):
            assert set(pc.elementwise_sizes(64, {2: 200, 6: 100, 12: 40}[d])) <= {len(b["a"]) for b in bs if b["op"] == op and b["rc"] == ZKT_OK}, (d, op)
    assert {b["nl"] for b in pc.fq12_pow_batches()} >= {1, 2, 3, 4, 8, 12}


def test_host_repeats_the_device_sequence_of_k_fp_op():
    """zkt_hostcheck_fp_canon repeats the 8-word branch of k_fp_op (the text is repeated, not shared, so that the product objects stay as they are): the two must not drift"""
    src = os.path.join(ROOT, "zk-toolkit_amd", "csrc")
    def body(fn):
        with open(os.path.join(src, fn)) as f: t = f.read()
        a = t.index("// canonical 32-bit-limb fields: any 256-bit input"); b = t.index("st_raw<C>(out + i * C::N, r);", a)
        return re.sub(r"\s+", "", t[a:b])
    assert body("zkt_field.hip") == body("hostcheck.cpp")


# ---- runners: one batch through one implementation -> (status, error index, outputs) ---------------------------------------------------------------
ORACLE_FIELD_OP = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "inv": 5, "cube": 6}
HOST_FIELD_OP = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "inv": 5, "cube": 7}
TOWER_OP = {"add": 0, "sub": 1, "mul": 2, "inv": 3, "neg": 4, "reduce": 5}


def _exp_words(b):
    """(exponent array, u64 limbs per exponent)"""
    if b["op"] == "pow": return pack([b["k"]] if b["shared"] else b["b"], b["exp_limbs"]), b["exp_limbs"]
    raise AssertionError(b["op"])


def field_oracle(b):
    f, w, op = FIELDS[b["pre"]]["id"], FIELDS[b["pre"]]["w"], b["op"]
    a = pack(b["a"], w); n = len(b["a"])
    if op in ORACLE_FIELD_OP:
        o = np.zeros_like(a); idx = ctypes.c_size_t(0)
        rc = O.zkto_field_op(f, ORACLE_FIELD_OP[op], ptr(a), ptr(pack(b["b"], w)), ptr(o), ctypes.c_size_t(n), ctypes.byref(idx))
        return rc, idx.value, unpack(o)
    if op == "pow":
        e, L = _exp_words(b); o = np.zeros_like(a)
        return O.zkto_field_pow_batch(f, ptr(a), ptr(e), L, b["shared"], ptr(o), ctypes.c_size_t(n)), None, unpack(o)
    if op == "scale":
        o = np.zeros_like(a)
        return O.zkto_field_op(f, 2, ptr(a), ptr(pack([b["k"]] * n, w)), ptr(o), ctypes.c_size_t(n), None), None, unpack(o)
    if op == "sum":                                                   # the oracle has the element-wise plus only: fold by halves (addition is exact in any order)
        cur = a
        while len(cur) > 1:
            h = len(cur) // 2; o = np.zeros((h, w), dtype=np.uint64)
            assert O.zkto_field_op(f, 0, ptr(np.ascontiguousarray(cur[:h])), ptr(np.ascontiguousarray(cur[h:2 * h])), ptr(o), ctypes.c_size_t(h), None) == 0
            cur = np.concatenate([o, cur[2 * h:]])
        z = np.zeros((1, w), dtype=np.uint64); o = np.zeros((1, w), dtype=np.uint64)
        assert O.zkto_field_op(f, 0, ptr(np.ascontiguousarray(cur)), ptr(z), ptr(o), ctypes.c_size_t(1), None) == 0      # + 0: a single term comes back reduced
        return 0, None, unpack(o)[0]
    o = np.zeros((b["n"], w), dtype=np.uint64)
    return O.zkto_field_pow_seq(f, ptr(a), ctypes.c_size_t(b["n"]), ptr(o), int(op == "repeat")), None, unpack(o)


def field_host(Hh, b):
    f, w, op = FIELDS[b["pre"]]["id"], FIELDS[b["pre"]]["w"], b["op"]
    a = pack(b["a"], w); n = len(b["a"])
    Hh.zkt_hostcheck_fp_canon.restype = _long; Hh.zkt_hostcheck_fp_first_zero.restype = _long
    if op in HOST_FIELD_OP:
        o = np.zeros_like(a); bb = pack(b["b"], w)
        if b["pre"] == "fq":                                           # the lazy-limb branch of k_fp_op: the zero test on the loaded value, then ld_fp / op / st_fp
            first = Hh.zkt_hostcheck_fp_first_zero(f, p32(a), ctypes.c_size_t(n)) if op == "inv" else -1
            if first < 0: assert Hh.zkt_hostcheck_fp(f, HOST_FIELD_OP[op], p32(a), p32(bb), p32(o), ctypes.c_size_t(n)) == 0
        else:
            first = Hh.zkt_hostcheck_fp_canon(f, HOST_FIELD_OP[op], p32(a), p32(bb), p32(o), ctypes.c_size_t(n))
            assert first >= -1
        return (ZKT_ERR_INV_ZERO, first, None) if first >= 0 else (0, None, unpack(o))
    vec = lambda vop, x, e, ew, sh, o, cnt: Hh.zkt_hostcheck_fp_vec(f, vop, p32(x), p32(e) if e is not None else None, ew, sh, p32(o), ctypes.c_size_t(cnt))
    if op == "pow":
        e, L = _exp_words(b); o = np.zeros_like(a)
        return vec(0, a, e, 2 * L, b["shared"], o, n), None, unpack(o)
    if op == "scale":
        o = np.zeros_like(a)
        return vec(1, a, pack([b["k"]], w), 0, 0, o, n), None, unpack(o)
    if op == "sum":
        o = np.zeros((1, w), dtype=np.uint64)
        return vec(2, a, None, 0, 0, o, n), None, unpack(o)[0]
    m = b["n"]; rep = np.repeat(a, m, axis=0); o = np.zeros((m, w), dtype=np.uint64)
    e = pack([1] * m if op == "repeat" else list(range(m)), 1)         # k_fp_pow_seq: base^i with a two-word exponent; repeat stores the loaded base
    return vec(0, rep, e, 2, 0, o, m), None, unpack(o)


def tower_oracle(b):
    d = b["deg"]; a, bb = pack_tower(b["a"]), pack_tower(b["b"]); o = np.zeros_like(a)
    rc = getattr(O, "zkto_fq%d_op" % d)(TOWER_OP[b["op"]], ptr(a), ptr(bb), ptr(o), ctypes.c_size_t(len(a)))
    return rc, None, unpack_tower(o, d)


def tower_host(Hh, b):
    d = b["deg"]; a, bb = pack_tower(b["a"]), pack_tower(b["b"]); o = np.zeros_like(a)
    Hh.zkt_hostcheck_tower_batch.restype = _long
    first = Hh.zkt_hostcheck_tower_batch(d, TOWER_OP[b["op"]], p32(a), p32(bb), p32(o), ctypes.c_size_t(len(a)))
    assert first >= -1
    return (ZKT_ERR_INV_ZERO, first, None) if first >= 0 else (0, None, unpack_tower(o, d))


def _e32(e, nl): return np.array([(e >> (32 * i)) & 0xFFFFFFFF for i in range(nl)], dtype=np.uint32)


def fq12_pow_oracle(b):
    a = pack_tower(b["a"]); o = np.zeros_like(a); e = _e32(b["e"], b["nl"])
    for i in range(len(a)):
        assert O.zkto_fq12_pow(ptr(a[i:i + 1]), p32(e), ctypes.c_size_t(b["nl"]), ptr(o[i:i + 1])) == 0
    return 0, None, unpack_tower(o, 12)


def fq12_pow_host(Hh, b):
    a = pack_tower(b["a"]); o = np.zeros_like(a)
    return Hh.zkt_hostcheck_fq12_pow(p32(a), p32(_e32(b["e"], b["nl"])), b["nl"], p32(o), ctypes.c_size_t(len(a))), None, unpack_tower(o, 12)


def group_oracle(b):
    grp, op = b["grp"], b["op"]; G = GROUPS[grp]; W = G["words"]
    a = pack_points(grp, b["pts"]); n = len(a)
    if op == "add":
        o = np.zeros_like(a)
        return getattr(O, "zkto_%s_add_batch" % grp)(ptr(a), ptr(pack_points(grp, b["pts_b"])), ptr(o), ctypes.c_size_t(n)), None, unpack_points(grp, o)
    if op == "neg":
        o = np.zeros_like(a)
        return getattr(O, "zkto_%s_neg_batch" % grp)(ptr(a), ptr(o), ctypes.c_size_t(n)), None, unpack_points(grp, o)
    if op in ("mul", "scale"):
        L = b["L"]
        if not 1 <= L <= 6: return None                                # the width check is the C ABI's; the oracle has none
        ks = b["ks"] * n if op == "scale" else b["ks"]
        o = np.zeros_like(a)
        return getattr(O, "zkto_%s_mul_batch" % grp)(ptr(a), ptr(pack(ks, L)), L, ptr(o), ctypes.c_size_t(n), 4), None, unpack_points(grp, o)
    if op == "sum":                                                   # the fold from infinity
        acc = pack_points(grp, [pc.ipt(None)])
        for i in range(n):
            o = np.zeros_like(acc)
            assert getattr(O, "zkto_%s_add_batch" % grp)(ptr(acc), ptr(np.ascontiguousarray(a[i:i + 1])), ptr(o), ctypes.c_size_t(1)) == 0
            acc = o
        return 0, None, unpack_points(grp, acc)[0]
    if op == "is_on_curve" and grp != "secp":
        return 0, None, [getattr(O, "zkto_%s_is_on_curve" % grp)(ptr(np.ascontiguousarray(a[i:i + 1]))) for i in range(n)]
    if op == "in_subgroup":                                           # order * P == infinity, with the oracle's scalar multiplication
        o = np.zeros_like(a); order = pack([G["order"]] * n, 4)
        assert getattr(O, "zkto_%s_mul_batch" % grp)(ptr(a), ptr(order), 4, ptr(o), ctypes.c_size_t(n), 4) == 0
        return 0, None, [int(p is None) for p in unpack_points(grp, o)]
    return None                                                        # is_on_curve for secp256k1: the oracle has no such entry; the host build and the device answer it


def group_host(Hh, b, lanes=1):
    grp, op = b["grp"], b["op"]; G = GROUPS[grp]
    a = pack_points(grp, b["pts"]); n = len(a)
    hb = lambda hop, bb, kw, ks, o, cnt: Hh.zkt_hostcheck_group_batch(G["id"], hop, p32(a), p32(bb) if bb is not None else None, kw, ks, p32(o), ctypes.c_size_t(cnt))
    if op == "add":
        o = np.zeros_like(a); return hb(0, pack_points(grp, b["pts_b"]), 0, 0, o, n), None, unpack_points(grp, o)
    if op == "neg":
        o = np.zeros_like(a); return hb(3, None, 0, 0, o, n), None, unpack_points(grp, o)
    if op in ("mul", "scale"):
        L = b["L"]
        if not 1 <= L <= 6: return None
        o = np.zeros_like(a); return hb(2, pack(b["ks"], L), 2 * L, 0 if op == "scale" else 2 * L, o, n), None, unpack_points(grp, o)
    if op == "sum":
        if n == 0: return None                                         # answered by the C ABI's host code without a kernel
        o = np.zeros((1, G["words"]), dtype=np.uint64); return hb(5, None, lanes, 0, o, n), None, unpack_points(grp, o)[0]
    if op == "is_on_curve":
        o = np.zeros(n, dtype=np.uint32); rc = hb(7, None, 0, 0, o, n); return rc, None, [int(v) for v in o]
    if op == "in_subgroup":
        o = np.zeros(n, dtype=np.uint32); rc = hb(4, pack([G["order"]], 4), 8, 0, o, n); return rc, None, [int(v) for v in o]
    return None


# ---- the case lists through the oracle and the host builds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(FIELDS))
def test_fields_oracle(pre):
    for b in pc.field_batches(pre): check(b, *field_oracle(b), who="oracle")


@pytest.mark.parametrize("pre", list(FIELDS))
def test_fields_host(H, pre):
    for b in pc.field_batches(pre): check(b, *field_host(H, b), who="host")


@pytest.mark.parametrize("deg", [2, 6, 12])
def test_tower_oracle(deg):
    for b in pc.tower_batches(deg): check(b, *tower_oracle(b), who="oracle")


@pytest.mark.parametrize("deg", [2, 6, 12])
def test_tower_host(H, deg):
    for b in pc.tower_batches(deg): check(b, *tower_host(H, b), who="host")


def test_fq12_pow_oracle():
    for b in pc.fq12_pow_batches(): check(b, *fq12_pow_oracle(b), who="oracle")


def test_fq12_pow_host(H):
    for b in pc.fq12_pow_batches(): check(b, *fq12_pow_host(H, b), who="host")


def _group_batches(grp):
    return pc.group_add_batches(grp) + pc.group_unary_batches(grp) + pc.group_mul_batches(grp) + pc.group_mul_geometry_batches(grp) + pc.group_sum_batches(grp)


@pytest.mark.parametrize("grp", list(GROUPS))
def test_groups_oracle(grp):
    for b in _group_batches(grp):
        r = group_oracle(b)
        if r is not None: check(b, *r, who="oracle")


@pytest.mark.parametrize("grp", list(GROUPS))
def test_groups_host(H, grp):
    for b in _group_batches(grp):
        for lanes in ((1, 2, 64) if b["op"] == "sum" else (1,)):       # a sum as the fold, and in the kernels' shape: strided lanes folded pairwise
            r = group_host(H, b, lanes)
            if r is not None: check(b, *r, who="host lanes=%d" % lanes)


def test_generator_comb_host(H):
    """the comb table of the generator and its digit walk (zkt_bls_public_keys_batch) on nibble patterns: zero nibbles are skipped, scalars are used as they are (k >= r included)"""
    cs = pc.comb_scalars()
    F = GROUPS["g1"]["F"]
    want = [pc.aff_mul(F, GROUPS["g1"]["gen"], k) for _, k in cs]
    gen = pack_points("g1", [pc.ipt(GROUPS["g1"]["gen"])]); o = np.zeros((len(cs), 13), dtype=np.uint64)
    assert H.zkt_hostcheck_group_batch(0, 6, p32(gen), p32(pack([k for _, k in cs], 4)), 8, 8, p32(o), ctypes.c_size_t(len(cs))) == 0
    check(dict(kind="comb", grp="g1", rc=ZKT_OK, want=want, labels=[l for l, _ in cs]), 0, None, unpack_points("g1", o), who="host")
