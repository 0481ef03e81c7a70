"""Every route of the pairing entry points against the python-integer model of tests/pairing_route_model.py — never against the oracle.

Batch sizes sit on both sides of each switch-over (zkt_tate_batch: 24,576 / 24,577; the product check: n K = 24,576 / 24,577 for K = 1..4; BLS:
12,288 / 12,289; Groth16: 8,192 / 8,193 proofs and n_stmt = 0, 1, 12, 13), and every batch carries elements of each class the model names at
lane 0, lanes 63 / 64, the last element, the last partial wave and, in the large batches, about one in 3,000 positions.  Every element is compared.
tests/test_pairing_route_model.py checks on the CPU that each cell of the model's ROUTES is reached by some call planned here.

Honest elements repeat a few pool pairs, so their expected values are a few dozen python exponentiations; each non-honest pair is one fixed pair
reused at many positions, so its plain-definition evaluation runs once.  The module skips itself when a switch-over limit is forced."""
import collections, ctypes, importlib, os
import numpy as np
import pytest
import pairing_route_model as M
from pairing_route_model import (HONEST, Q_TWIST, Q_OFF, P_OUT_VALUE, P_OUT_PANIC, P_OFF, P_OUT_Q_TWIST, INF, g1, g2, g2_twist, g2_off, g1_out,
                                 g1_off, g1_order3, G1_INF)
from zkt_testlib import R, G1W, G2W, FQ12, SplitMix64, ptr, ints_to_arr

FORCED = bool(os.environ.get("ZKT_DTATE_MAX") or os.environ.get("ZKT_DPRODUCT_MAX"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="a forced switch-over limit moves every route this module claims")]

_rng = SplitMix64(0x5EED)
A_LOGS = [_rng.below(R - 1) + 1 for _ in range(8)]
B_LOGS = [_rng.below(R - 1) + 1 for _ in range(8)]


# ---- one fixed pair per non-honest class (tests/pairing_route_model.py builds them from python integers) ----
def class_pair(cls):
    return {Q_TWIST: lambda: (g1(A_LOGS[0]), g2_twist(B_LOGS[1])), Q_OFF: lambda: (g1(A_LOGS[1]), g2_off(B_LOGS[2])),
            P_OUT_VALUE: lambda: (g1_out(A_LOGS[2]), g2(B_LOGS[3])), P_OFF: lambda: (g1_off(A_LOGS[3]), g2(B_LOGS[4])),
            P_OUT_Q_TWIST: lambda: (g1_out(A_LOGS[2]), g2_twist(B_LOGS[5])), P_OUT_PANIC: lambda: (g1_order3(), g2(B_LOGS[0])),
            INF: lambda: (G1_INF, g2(B_LOGS[0]))}[cls]()


MARKED = (Q_TWIST, Q_OFF, P_OUT_VALUE, P_OFF, P_OUT_Q_TWIST)


def special_positions(n):
    """lane 0, lanes 63 / 64, the last element, the last partial wave, and about one in 3,000 positions"""
    pos = {0, 63, 64, n - 1}
    if n % 64:
        pos.add(n - 1 - (n % 64) // 2)
    pos.update(range(1499, n, 3000))
    return sorted(p for p in pos if p < n)


def layout(n, n_honest, marked):
    """template index per position: honest templates 0..n_honest-1 in turn, marked templates n_honest.. at the special positions, in turn"""
    lay = np.arange(n) % n_honest
    for k, p in enumerate(special_positions(n)):
        lay[p] = n_honest + (k + n) % marked if marked else lay[p]
    return lay


# ---- zkt_tate_batch -----------------------------------------------------------------------------------------------------------------
TATE_NS = (1, 5, 6, 11, 12, 13, 64, 65, 24576, 24577)


def plan_tate(n):
    honest = [(g1(A_LOGS[i % 8]), g2(B_LOGS[(i // 8) % 8])) for i in range(16)]
    templates = honest + [class_pair(c) for c in MARKED]
    return templates, layout(n, len(honest), len(MARKED))


def plan_tate_panics(n, lo, hi, chain_first):
    templates, lay = plan_tate(n)
    templates = templates + [class_pair(P_OUT_PANIC), class_pair(INF)]
    lay = lay.copy()
    lay[lo], lay[hi] = (len(templates) - 2, len(templates) - 1) if chain_first else (len(templates) - 1, len(templates) - 2)
    return templates, lay


def tate_cells(n, templates, lay):
    return {("tate", M.tate_route(n), M.tate_pass(*templates[t])) for t in set(lay.tolist())}


def tate_arrays(templates, lay):
    P = M.g1_rows([p for p, _ in templates])[lay]
    Qs = M.g2_rows([q for _, q in templates])[lay]
    return np.ascontiguousarray(P), np.ascontiguousarray(Qs)


def tate_expected(templates, lay):
    rc, idx, vals = M.tate_call(templates)
    words = np.stack([M.gt_words(v) if v is not None else np.zeros(FQ12, np.uint64) for v in vals])
    panics = [p for p in range(len(lay)) if vals[lay[p]] is None]
    return (2 if panics else 0), (min(panics) if panics else None), words[lay]


zk = importlib.import_module("zk-toolkit_amd")


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def _tate_run(L, P, Qs, dev):
    n = P.shape[0]
    out = np.zeros((n, FQ12), np.uint64)
    if not dev:
        return L.zkt_tate_batch(ptr(P), ptr(Qs), ptr(out), ctypes.c_size_t(n)), out
    import torch
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dP, dQ = torch.from_numpy(P.view(np.int64)).cuda(), torch.from_numpy(Qs.view(np.int64)).cuda()
    dO = torch.zeros((n, FQ12), dtype=torch.int64, device="cuda")
    rc = L.zkt_tate_batch_dev(vp(dP), vp(dQ), vp(dO), ctypes.c_size_t(n), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, dO.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n", TATE_NS)
def test_tate_routes_every_element(L, n, dev):
    templates, lay = plan_tate(n)
    rc_want, _, want = tate_expected(templates, lay)
    P, Qs = tate_arrays(templates, lay)
    rc, got = _tate_run(L, P, Qs, dev)
    assert rc == rc_want == 0
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(i), M.classify(*templates[lay[i]])) for i in bad[:8]]


@pytest.mark.parametrize("chain_first", [True, False], ids=["chain-low", "inf-low"])
@pytest.mark.parametrize("n", [64, 24577])
def test_tate_two_panics_from_different_passes(L, n, chain_first):
    lo, hi = 5, n - 2
    templates, lay = plan_tate_panics(n, lo, hi, chain_first)
    rc_want, idx_want, _ = tate_expected(templates, lay)
    assert (rc_want, idx_want) == (2, lo)
    P, Qs = tate_arrays(templates, lay)
    rc, _ = _tate_run(L, P, Qs, False)
    assert rc == 2 and L.zkt_last_error_index() == lo


# ---- zkt_pairing_product_check_batch ------------------------------------------------------------------------------------------------
NEG_PATTERNS = {"none": (0, 0, 0, 0), "all": (1, 1, 1, 1), "mixed": (0, 1, 1, 0)}
PRODUCT_CASES = [(K, neg, n) for K in (1, 2, 3, 4) for neg in NEG_PATTERNS for n in (5, M.DPRODUCT_MAX // K, M.DPRODUCT_MAX // K + 1)]


def _sgn(neg):
    return -1 if neg else 1


def _accept(K, neg, seed, twist_slot=None):
    """K honest pairs with sum of +-a b = 0 mod r (the last G1 log solves it); twist_slot: that slot's Q carries a cofactor component (same log)"""
    bs = [B_LOGS[(seed + j) % 8] for j in range(K)]
    as_ = [A_LOGS[(seed + 3 * j) % 8] for j in range(K - 1)]
    rest = sum(_sgn(neg[j]) * as_[j] * bs[j] for j in range(K - 1))
    if K == 1:                                                   # e(P, Q) = 1 needs a log 0: the cofactor point alone (a reject otherwise)
        bs = [0] if twist_slot == 0 else bs
        as_ = [A_LOGS[seed % 8]]
    else:
        as_.append(-rest * _sgn(neg[K - 1]) * pow(bs[K - 1], -1, R) % R)
    q = [g2_twist(b) if j == twist_slot else g2(b) for j, b in enumerate(bs)]
    return [(g1(a), qq) for a, qq in zip(as_, q)]


def _twin(pairs):
    """the same element one unit off in the last slot's G1 log (or, for a cofactor-only Q, its G2 log)"""
    p, q = pairs[-1]
    if q.kind == "twist" and q.log == 0:
        return pairs[:-1] + [(p, g2_twist(1))]
    return pairs[:-1] + [(g1(p.log + 1), q)]


def plan_product(K, neg_name, n, panics=None):
    neg = list(NEG_PATTERNS[neg_name][:K])
    honest = []
    for s in range(3):
        if K > 1:
            acc = _accept(K, neg, s)
            honest += [acc, _twin(acc)]
        acc = _accept(K, neg, s + 5, twist_slot=0)               # the 255-step loop (OK_REDO), accepting, and its rejected twin
        honest += [acc, _twin(acc)]
    out_pair, off_pair = class_pair(P_OUT_VALUE), class_pair(Q_OFF)
    marked = [[out_pair] + _accept(K, neg, 7)[1:]]               # P outside G1 in slot 0 (negated or not by the pattern)
    if K > 1:
        one = [(g1(A_LOGS[j]), g2_twist(0)) for j in range(2, K)]            # T^0 = 1 whatever the G1 log
        marked.append([out_pair, out_pair] + one)               # the same pair on both sides when slots 0 and 1 differ in sign: the reference accepts
        marked.append(_accept(K, neg, 8)[:1] + [out_pair] + _accept(K, neg, 8)[2:])
    marked.append(_accept(K, neg, 9)[:-1] + [off_pair])          # Q off its curve in the last slot
    templates = honest + marked
    lay = layout(n, len(honest), len(marked))
    if panics:
        templates = templates + [[class_pair(P_OUT_PANIC)] + _accept(K, neg, 4)[1:], [(G1_INF, g2(B_LOGS[0]))] + _accept(K, neg, 4)[1:]]
        lo, hi, chain_first = panics
        lay = lay.copy()
        lay[lo], lay[hi] = (len(templates) - 2, len(templates) - 1) if chain_first else (len(templates) - 1, len(templates) - 2)
    return templates, lay, neg


def product_expected(templates, lay, neg, fail_closed=False):
    rc, _, passes, oks = M.product_call(templates, neg, fail_closed)
    panics = [p for p in range(len(lay)) if passes[lay[p]] in (M.INF_PANIC, M.EXACT_PANIC)]
    ok = np.array([-1 if o is None else o for o in oks], np.int64)[lay]
    return (2 if panics else 0), (min(panics) if panics else None), passes, ok


def product_arrays(templates, lay):
    K = len(templates[0])
    P = np.stack([M.g1_rows([p for p, _ in t]) for t in templates])[lay].reshape(-1, G1W)
    Qs = np.stack([M.g2_rows([q for _, q in t]) for t in templates])[lay].reshape(-1, G2W)
    return np.ascontiguousarray(P), np.ascontiguousarray(Qs), K


def _product_run(L, templates, lay, neg):
    P, Qs, K = product_arrays(templates, lay)
    n = len(lay)
    ok = np.zeros(n, np.uint32)
    rc = L.zkt_pairing_product_check_batch(ptr(P), ptr(Qs), np.array(neg, np.uint8).ctypes.data_as(ctypes.c_void_p), K, n,
                                           ok.ctypes.data_as(ctypes.c_void_p))
    return rc, ok


def product_calls(K, neg_name, n):
    """(fail_closed, panics) of every call a product case makes"""
    return [(False, None), (True, None), (False, (1 % n, n - 1, True)), (True, (1 % n, n - 1, True)), (False, (1 % n, n - 1, False))] if n > 2 else \
           [(False, None), (True, None)]


def product_cells(K, neg_name, n):
    cells = set()
    for fc, pn in product_calls(K, neg_name, n):
        templates, lay, neg = plan_product(K, neg_name, n, pn)
        _, _, passes, _ = product_expected(templates, lay, neg, fc)
        cells |= {("product", M.product_route(n, K), passes[t]) for t in set(lay.tolist())}
    return cells


@pytest.mark.parametrize("K,neg_name,n", PRODUCT_CASES, ids=[f"K{K}-{g}-n{n}" for K, g, n in PRODUCT_CASES])
def test_product_check_routes(L, K, neg_name, n):
    for fc, pn in product_calls(K, neg_name, n):
        templates, lay, neg = plan_product(K, neg_name, n, pn)
        rc_want, idx_want, _, ok_want = product_expected(templates, lay, neg, fc)
        L.zkt_verify_set_fail_closed(1 if fc else 0)
        try:
            rc, ok = _product_run(L, templates, lay, neg)
        finally:
            L.zkt_verify_set_fail_closed(0)
        assert rc == rc_want, (fc, pn)
        if rc:
            assert L.zkt_last_error_index() == idx_want, (fc, pn)
            continue
        bad = np.nonzero(ok.astype(np.int64) != ok_want)[0]
        assert bad.size == 0, (fc, [(int(i), int(lay[i]), int(ok[i]), int(ok_want[i])) for i in bad[:8]])
        if not pn and not fc and n >= 64:                        # both verdicts occur (smaller batches hold marked elements almost only)
            assert ok_want.min() == 0 and ok_want.max() == 1


# ---- zkt_bls_verify_batch: K = 2, the generator as a trusted shared G1 point on the large path ----------------------------------------
BLS_NS = (12288, 12289)
_MSGS = [b"route model %d" % i for i in range(4)]
_SKS = [_rng.below(R - 1) + 1 for _ in range(4)]


def plan_bls(n):
    hs = [int.from_bytes(m, "big") % R for m in _MSGS]
    templates, meta = [], []
    for i in range(16):
        sk, j = _SKS[i % 4], i // 4
        templates.append([(g1(1), g2(sk * hs[j])), (g1(sk), g2(hs[j]))]); meta.append((i % 4, j, i % 4))
    for i in range(4):                                           # forged: the signature of another message, or of another key
        sk, j = _SKS[i], (i + 1) % 4
        templates.append([(g1(1), g2(sk * hs[(j + 1) % 4])), (g1(sk), g2(hs[j]))]); meta.append((i, j, i))
    lay = layout(n, 16, 4)
    return templates, lay, meta


def bls_cells(n):
    templates, lay, _ = plan_bls(n)
    return {("bls", M.product_route(n, 2), M.product_pass(templates[t])) for t in set(lay.tolist())}


@pytest.mark.parametrize("n", BLS_NS)
def test_bls_batch_routes(L, n):
    templates, lay, meta = plan_bls(n)
    _, _, passes, oks = M.product_call(templates, [0, 1])
    want = np.array(oks, np.int64)[lay]
    assert set(passes) == {M.ATE} and want.min() == 0 and want.max() == 1
    msgs = b"".join(_MSGS[meta[t][1]] for t in lay)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(_MSGS[meta[t][1]]) for t in lay])
    sigs = np.ascontiguousarray(M.g2_rows([t[0][1] for t in templates])[lay])
    pks = np.ascontiguousarray(M.g1_rows([t[1][0] for t in templates])[lay])
    ok = np.zeros(n, np.uint32)
    buf = np.frombuffer(msgs, np.uint8).copy()
    assert L.zkt_bls_verify_batch(buf.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p), ptr(sigs), ptr(pks), n,
                                  ok.ctypes.data_as(ctypes.c_void_p)) == 0
    bad = np.nonzero(ok.astype(np.int64) != want)[0]
    assert bad.size == 0, [(int(i), int(lay[i])) for i in bad[:8]]


# ---- zkt_groth16_verify_batch / zkt_groth16_verify ----------------------------------------------------------------------------------
L_STMT = 12                                                      # l = 12: 13 statement points, so n_stmt = 13 is a legal shape
_U = [_rng.below(R - 1) + 1 for _ in range(L_STMT + 1)]
_BETA, _GAMMA, _DELTA = (_rng.below(R - 1) + 1 for _ in range(3))


def make_key(alpha, kind="honest"):
    gamma = g2_twist(_GAMMA) if kind == "gamma-twist" else g2(_GAMMA)
    kappa = alpha * _BETA + (1 if kind == "wrong-gt" else 0)
    return M.Key(alpha, _BETA, gamma, g2(_DELTA), _U, kappa=kappa, null_alpha_beta=(kind == "null-alpha-beta"))


def crs_for(key):
    from qap_util import alloc_crs
    c, buf = alloc_crs(1, L_STMT, L_STMT)
    buf["g1_alpha"][:] = M.g1_rows([g1(key.alpha)]); buf["g2_beta"][:] = M.g2_rows([g2(key.beta)])
    buf["g2_gamma"][:] = M.g2_rows([key.gamma]); buf["g2_delta"][:] = M.g2_rows([key.delta])
    buf["g1_uvw_stmt"][:] = M.g1_rows([g1(u) for u in key.u]); buf["gt_alpha_beta"][:] = M.gt_words(M.gt(key.kappa))
    if key.null_alpha_beta:
        c.g1_alpha = None; c.g2_beta = None
    return c, buf


def _proof(key, n_stmt, seed, forged=False, b_twist=False):
    rng = SplitMix64(1000 + seed)
    a, b = A_LOGS[seed % 8], B_LOGS[(seed + 3) % 8]
    stmt = [rng.below(R - 1) + 1 for _ in range(n_stmt)]
    s = sum(x * u for x, u in zip(stmt, key.u))
    c = (a * b - key.kappa - s * key.gamma.log) * pow(key.delta.log, -1, R) % R
    return (g1(a), g2_twist(b) if b_twist else g2(b), g1(c + (1 if forged else 0)), stmt)


def plan_groth16(key, n_stmt, n, panics=None):
    honest = []
    for s in range(3):
        honest += [_proof(key, n_stmt, s), _proof(key, n_stmt, s, forged=True)]
    marked = [_proof(key, n_stmt, 3, b_twist=True), _proof(key, n_stmt, 3, forged=True, b_twist=True)]
    out_a, out_b = class_pair(P_OUT_VALUE)
    h = _proof(key, n_stmt, 4)
    marked.append((out_a, out_b, h[2], h[3]))                    # A outside G1
    marked.append((h[0], h[1], out_a, h[3]))                     # C outside G1
    templates = honest + marked
    lay = layout(n, len(honest), len(marked))
    if panics:
        lo, hi, chain_first = panics
        chain = (g1_order3(), h[1], h[2], h[3])
        zero = (h[0], h[1], h[2], [0] * n_stmt)                  # S = infinity: the reference's tate(sum, gamma) panics
        templates = templates + ([chain, zero] if n_stmt else [chain])
        lay = lay.copy()
        if n_stmt:
            lay[lo], lay[hi] = (len(templates) - 2, len(templates) - 1) if chain_first else (len(templates) - 1, len(templates) - 2)
        else:
            lay[lo] = len(templates) - 1
    return templates, lay


def groth16_expected(key, route, templates, lay, fail_closed=False):
    rc, _, passes, oks = M.groth16_call(key, route, templates, fail_closed)
    panics = [p for p in range(len(lay)) if passes[lay[p]] in (M.INF_PANIC, M.EXACT_PANIC)]
    ok = np.array([-1 if o is None else o for o in oks], np.int64)[lay]
    return (2 if panics else 0), (min(panics) if panics else None), passes, ok


def _groth16_run(L, crs, templates, lay, n_stmt, single_too=False):
    n = len(lay)
    A = np.ascontiguousarray(M.g1_rows([t[0] for t in templates])[lay]); B = np.ascontiguousarray(M.g2_rows([t[1] for t in templates])[lay])
    C = np.ascontiguousarray(M.g1_rows([t[2] for t in templates])[lay])
    W = np.ascontiguousarray(np.stack([ints_to_arr(t[3], 4) if n_stmt else np.zeros((0, 4), np.uint64) for t in templates])[lay].reshape(-1, 4))
    ok = np.zeros(n, np.uint32)
    rc = L.zkt_groth16_verify_batch(ctypes.byref(crs), ptr(A), ptr(B), ptr(C), ptr(W) if n_stmt else None, n_stmt, n, ok.ctypes.data_as(ctypes.c_void_p))
    single = L.zkt_groth16_verify(ctypes.byref(crs), ptr(A[-1:].copy()), ptr(B[-1:].copy()), ptr(C[-1:].copy()), ptr(W[-n_stmt:].copy()) if n_stmt else None, ctypes.c_size_t(n_stmt)) \
        if rc == 0 and single_too else None
    return rc, ok, single


GROTH16_CASES = [(ns, n) for ns in (1, 12, 13) for n in (1, 6, 8192, 8193)]
UNSERVABLE_CASES = [(kind, n) for kind in ("gamma-twist", "wrong-gt", "null-alpha-beta") for n in (6, 8193)]


def groth16_calls(key, n_stmt, n):
    """(label, cached, fail_closed, panics) of every call in order: first sight, again, after zkt_groth16_vk_prepare, panics and fail-closed on
    the cached key, then (after four other keys) first sight again"""
    pn = (n // 3, n - 1, True) if n > 1 else (0, 0, True)
    pn2 = (n // 3, n - 1, False) if n > 1 else None
    calls = [("first", False, False, None), ("again", True, False, None), ("prepared", True, False, None), ("panics", True, False, pn),
             ("fail-closed", True, True, None)]
    if pn2:
        calls.append(("panics-swapped", True, False, pn2))
    calls.append(("evicted", False, False, None))
    return calls


def groth16_cells(key, n_stmt, n):
    cells = set()
    for label, cached, fc, pn in groth16_calls(key, n_stmt, n):
        route = M.groth16_route(key, n_stmt, n, cached)
        templates, lay = plan_groth16(key, n_stmt, n, pn)
        _, _, passes, _ = groth16_expected(key, route, templates, lay, fc)
        cells |= {("groth16", route, passes[t]) for t in set(lay.tolist())}
    return cells


_alpha_seed = [0]


def _fresh_alpha():
    _alpha_seed[0] += 1
    return SplitMix64(77 + _alpha_seed[0]).below(R - 1) + 1


def _evict(L):
    """four keys the process has not seen: every entry of the four-key cache is replaced"""
    for _ in range(4):
        k = make_key(_fresh_alpha())
        crs, buf = crs_for(k)
        A, B, C, stmt = _proof(k, 1, 0)
        assert L.zkt_groth16_verify(ctypes.byref(crs), ptr(M.g1_rows([A])), ptr(M.g2_rows([B])), ptr(M.g1_rows([C])), ptr(ints_to_arr(stmt, 4)), ctypes.c_size_t(1)) == 1


def _groth16_sequence(L, key, n_stmt, n):
    crs, buf = crs_for(key)
    oks = {}
    for label, cached, fc, pn in groth16_calls(key, n_stmt, n):
        if label == "prepared":
            assert L.zkt_groth16_vk_prepare(ctypes.byref(crs), ctypes.c_size_t(n_stmt)) == 0
        if label == "evicted":
            _evict(L)
        route = M.groth16_route(key, n_stmt, n, cached)
        templates, lay = plan_groth16(key, n_stmt, n, pn)
        rc_want, idx_want, _, ok_want = groth16_expected(key, route, templates, lay, fc)
        L.zkt_verify_set_fail_closed(1 if fc else 0)
        try:
            rc, ok, single = _groth16_run(L, crs, templates, lay, n_stmt, single_too=cached)      # (a single proof at first sight would itself cache the key)
        finally:
            L.zkt_verify_set_fail_closed(0)
        assert rc == rc_want, label
        if rc:
            assert L.zkt_last_error_index() == idx_want, label
            continue
        bad = np.nonzero(ok.astype(np.int64) != ok_want)[0]
        assert bad.size == 0, (label, route, [(int(i), int(lay[i]), int(ok[i]), int(ok_want[i])) for i in bad[:8]])
        assert single is None or single == ok_want[-1], label
        oks.setdefault(fc, []).append(ok.copy())
    for fc, vs in oks.items():
        assert all((v == vs[0]).all() for v in vs), fc
    assert n == 1 or (oks[False][0].max() == 1 and oks[False][0].min() == 0)


@pytest.mark.parametrize("n_stmt,n", GROTH16_CASES, ids=[f"stmt{a}-n{b}" for a, b in GROTH16_CASES])
def test_groth16_key_routes(L, n_stmt, n):
    _groth16_sequence(L, make_key(_fresh_alpha()), n_stmt, n)


@pytest.mark.parametrize("kind,n", UNSERVABLE_CASES, ids=[f"{a}-n{b}" for a, b in UNSERVABLE_CASES])
def test_groth16_keys_the_ate_route_must_not_serve(L, kind, n):
    key = make_key(_fresh_alpha(), kind)
    assert not key.servable(1)
    _groth16_sequence(L, key, 1, n)


@pytest.mark.parametrize("n", [1, 6, 8192, 8193])
def test_groth16_without_statement_panics_at_the_first_proof(L, n):
    """n_stmt = 0: the statement sum is infinity, and the reference's tate(sum, gamma) panics for every proof (verifier.rs:41-47)"""
    key = make_key(_fresh_alpha())
    templates, lay = plan_groth16(key, 0, n)
    rc_want, idx_want, passes, _ = groth16_expected(key, M.groth16_route(key, 0, n, False), templates, lay)
    assert (rc_want, idx_want) == (2, 0) and set(passes) == {M.INF_PANIC}
    crs, buf = crs_for(key)
    rc, _, _ = _groth16_run(L, crs, templates, lay, 0)
    assert rc == 2 and L.zkt_last_error_index() == 0


def all_cells():
    """Counter: (entry point, batch route, element pass) -> how many cases of this module reach it, by the model"""
    cells = collections.Counter()
    for n in TATE_NS:
        cells.update(tate_cells(n, *plan_tate(n)))
    for n in (64, 24577):
        for cf in (True, False):
            cells.update(tate_cells(n, *plan_tate_panics(n, 5, n - 2, cf)))
    for case in PRODUCT_CASES:
        cells.update(product_cells(*case))
    for n in BLS_NS:
        cells.update(bls_cells(n))
    for ns, n in GROTH16_CASES:
        cells.update(groth16_cells(make_key(2), ns, n))
    for kind, n in UNSERVABLE_CASES:
        cells.update(groth16_cells(make_key(2, kind), 1, n))
    for n in (1, 6, 8192, 8193):
        key = make_key(2)
        route = M.groth16_route(key, 0, n, False)
        templates, lay = plan_groth16(key, 0, n)
        _, _, passes, _ = groth16_expected(key, route, templates, lay)
        cells.update({("groth16", route, passes[t]) for t in set(lay.tolist())})
    return cells
