"""CPU checks of the pairing route model (tests/pairing_route_model.py): its switch-over limits are the library's, its predicted pass for every element
class agrees with the host build of the device code, its python values and decisions equal the oracle's on a sample of each class, and every cell of
its ROUTES is reached by some call of tests/test_gpu_pairing_routes.py — all before anything runs on a GPU."""
import ctypes
import numpy as np
import pytest
import pairing_route_model as M
import test_gpu_pairing_routes as G
from zkt_testlib import R, FQ12, ptr, fq12_from_arr, oracle
from test_hostcheck import H, p32, _u32p                          # noqa: F401  (H: the two host builds of the kernel headers)
from test_oracle_pairing import pair


def test_switch_over_limits_are_the_library_defaults():
    assert M.library_limits() == {"ZKT_DTATE_MAX": M.DTATE_MAX, "ZKT_DPRODUCT_MAX": M.DPRODUCT_MAX}


def _sample():
    """one pair of every class the GPU module uses, and a second of the classes built from several pieces"""
    pairs = [(c, G.class_pair(c)) for c in G.MARKED + (M.P_OUT_PANIC, M.INF)]
    pairs.append((M.HONEST, (M.g1(G.A_LOGS[5]), M.g2(G.B_LOGS[6]))))
    pairs.append((M.Q_TWIST, (M.g1(G.A_LOGS[4]), M.g2_twist(0))))
    pairs.append((M.P_OFF, (M.g1_off(G.A_LOGS[6]), M.g2(G.B_LOGS[7]))))
    return pairs


def test_classes_are_what_the_gpu_module_says():
    for cls, (p, q) in _sample():
        assert M.classify(p, q) == cls


def test_predicted_passes_agree_with_the_host_build(H):
    H.zkt_hostcheck_short_loop_guards.argtypes = [_u32p, _u32p]
    H.zkt_hostcheck_ate_product.argtypes = [ctypes.c_int, ctypes.c_int, _u32p, _u32p, _u32p]
    for cls, (p, q) in _sample():
        P, Qa = M.g1_rows([p]), M.g2_rows([q])
        got = np.zeros((1, FQ12), np.uint64)
        ps = M.tate_pass(p, q)
        assert H.zkt_hostcheck_tate(p32(P), p32(Qa), p32(got)) == M.HOSTCHECK_TATE[ps], (cls, ps)
        v = M.pair_value(p, q)
        if v is not None:
            assert (got[0] == M.gt_words(v)).all(), cls                # the host build's value: the model's, bit for bit
        if cls == M.INF:
            continue
        bits, mask = M.short_loop_guards(p, q)
        assert H.zkt_hostcheck_short_loop_guards(p32(P), p32(Qa)) & mask == bits & mask, cls
        assert (H.zkt_hostcheck_ate_product(1, 0, p32(P), p32(Qa), p32(got)) == -1) == (M.product_pass([(p, q)]) != M.ATE), cls


def test_values_equal_the_oracle_on_every_class():
    """the plain-definition chain (panics included), bilinearity for the in-group arguments, T = the SURVEY Appendix B value the oracle pins"""
    for cls, (p, q) in _sample() + [(M.HONEST, (M.g1(1), M.g2(1)))]:
        rc, want, _ = pair(3, M.g1_rows([p]), M.g2_rows([q]), threads=1)
        v = M.pair_value(p, q)
        assert (rc != 0) == (v is None), cls
        if v is not None:
            assert tuple(fq12_from_arr(want)[0]) == tuple(M.fm.to_ref_order(v)), cls


def test_decisions_equal_the_oracle():
    """the discrete-log rule and the two-sided exact rule against the oracle: its pairings multiplied the reference's way, and its Groth16 verifier
    on a key built from logs (honest, forged, B on the twist, A outside G1, a wrong stored alpha_beta)"""
    O = oracle()

    def gtmul(a, b):
        o = np.zeros((1, FQ12), np.uint64)
        assert O.zkto_fq12_op(2, ptr(a), ptr(b), ptr(o), 1) == 0
        return o

    one = np.zeros((1, FQ12), np.uint64); one[0, 66] = 1
    for K, neg_name in ((2, "mixed"), (3, "none"), (4, "all")):
        templates, lay, neg = G.plan_product(K, neg_name, 5)
        for t in templates:
            ps, ok = M.product_ok(t, neg)
            if ps == M.EXACT_PANIC:
                continue
            side = [one.copy(), one.copy()]
            for (p, q), n in zip(t, neg):
                rc, v, _ = pair(3, M.g1_rows([p]), M.g2_rows([q]), threads=1)
                assert rc == 0
                side[n] = gtmul(side[n], v)
            assert ok == int((side[0] == side[1]).all()), (K, neg_name, ps)
    for kind in ("honest", "wrong-gt"):
        key = G.make_key(3, kind)
        crs, buf = G.crs_for(key)
        templates, _ = G.plan_groth16(key, 2, 5)
        for A, B, C, stmt in templates:
            _, ok = M.groth16_ok(key, "small/127", A, B, C, stmt)
            want = O.zkto_groth16_verify(ctypes.byref(crs), ptr(M.g1_rows([A])), ptr(M.g2_rows([B])), ptr(M.g1_rows([C])), ptr(G.ints_to_arr(stmt, 4)), 2)
            assert want == ok, (kind, A.kind, B.kind, C.kind)


def test_every_route_cell_is_reached_by_the_gpu_module():
    count = G.all_cells()
    missing = [c for c in M.ROUTES if not count[c]]
    unknown = sorted(c for c in count if c not in M.ROUTES)
    for c in M.ROUTES:
        print("route cell", c, "reached by", count[c], "cases")
    assert not missing and not unknown, (missing, unknown)


def test_the_limits_decide_the_boundary_cases():
    """each boundary size of the GPU module lies on the side of the limit it is named for"""
    assert M.tate_route(24576) == "k_dtate" and M.tate_route(24577) == "k_tate"
    for K in (1, 2, 3, 4):
        n = M.DPRODUCT_MAX // K
        assert n * K == M.DPRODUCT_MAX and M.product_route(n, K) == "k_dproduct_ate" and M.product_route(n + 1, K) == "k_pairing_product_check_ate"
    key = G.make_key(3)
    assert M.groth16_route(key, 1, 8192, True) == "small/ate" and M.groth16_route(key, 1, 8193, False) == "large/ate"
    assert M.groth16_route(key, 13, 6, True) == "large/127" and M.groth16_route(key, 0, 6, True) == "large/127"
    assert M.groth16_route(key, 12, 6, False) == "small/127"
