"""CPU checks of tests/dense_model.py: its exponents, multiplied onto the generators, are the oracle's line-by-line restatement of both dense protocols at the
reference's toy circuits (which ties the model to the reference); its constants are the ones the library source holds; and the case lists of
tests/test_gpu_dense_protocols.py reach every cell of CELLS — checked before anything runs on a GPU."""
import ctypes, os, re
import numpy as np
import pytest
import dense_model as D
from zkt_testlib import oracle, ptr, ints_to_arr, SplitMix64, R, G1W, G2W, FQ12
from qap_util import (example_cubic, chain_circuit, chain_io_circuit, qap_from_r1cs, pinocchio_instance, alloc_crs, alloc_pinocchio, alloc_pinocchio_proof, poly_mul)

O = oracle()
fr = lambda v: ints_to_arr([v], 4)
flat = lambda polys, n: [c for p in polys for c in (list(p) + [0] * (n - len(p)))]


def _circuit(case):
    return example_cubic() if case == "cubic" else chain_circuit(int(case[5:]))      # cubic: the reference's own test (prover.rs:159-192)


def _same(got, group, scalars, what):
    want = D.expected_points(O, group, scalars)
    assert got[:len(scalars)].tobytes() == want.tobytes(), what


@pytest.mark.parametrize("case", ["cubic", "chain4"])
def test_groth16_model_equals_the_oracle_s_restatement(case):
    A, B, C, wit, l = _circuit(case)
    n, m = len(A), len(wit) - 1
    ui, vi, wi, h, _ = qap_from_r1cs(A, B, C, wit)
    U, V, W = flat(ui, n), flat(vi, n), flat(wi, n)
    rng = SplitMix64(900 + n)
    trap = [rng.below(R - 1) + 1 for _ in range(5)]
    r, s = rng.below(R - 1) + 1, rng.below(R - 1) + 1
    crs, buf = alloc_crs(n, l, m)
    assert O.zkto_groth16_setup(ctypes.byref(crs), ptr(ints_to_arr(U, 4)), ptr(ints_to_arr(V, 4)), ptr(ints_to_arr(W, 4)), *[ptr(fr(t)) for t in trap]) == 0
    model = D.groth16_crs(U, V, W, n, l, m, *trap)
    assert sorted(model) == sorted(D.G16_GROUPS) and len(model) + 1 == len(buf)
    for name, scalars in model.items():
        _same(buf[name], D.G16_GROUPS[name], scalars, name)
    gt = np.zeros((1, FQ12), np.uint64)
    assert O.zkto_pairing_batch(3, ptr(D.expected_points(O, "g1", model["g1_alpha"])), ptr(D.expected_points(O, "g2", model["g2_beta"])), ptr(gt), 1, 1, None) == 0
    assert gt.tobytes() == buf["gt_alpha_beta"].tobytes()
    out = {"A": np.zeros((1, G1W), np.uint64), "B": np.zeros((1, G2W), np.uint64), "C": np.zeros((1, G1W), np.uint64)}
    for h_len in sorted({0, 1, len(h)}):
        assert O.zkto_groth16_prove(ctypes.byref(crs), ptr(ints_to_arr(U, 4)), ptr(ints_to_arr(V, 4)), ptr(ints_to_arr(wit, 4)), ptr(ints_to_arr(h, 4)), h_len,
                                    ptr(fr(r)), ptr(fr(s)), int(h_len == len(h)), *[ptr(out[k]) for k in "ABC"]) == 0      # the reference's per-wire loop once
        proof = D.groth16_proof(model, U, V, wit, h[:h_len], r, s, n, l, m)
        for k in "ABC":
            _same(out[k], D.PROOF16_GROUPS[k], [proof[k]], (k, h_len))


@pytest.mark.parametrize("case", ["cubic", "chain4"])
def test_pinocchio_model_equals_the_oracle_s_restatement(case):
    A, B, C, wit, l = _circuit(case)
    n, n_io = len(A), l + 1
    n_mid = len(wit) - n_io
    vi, wi, yi, h, _ = qap_from_r1cs(A, B, C, wit)
    V, W, Y = flat(vi, n), flat(wi, n), flat(yi, n)
    max_degree = pinocchio_instance(A, B, C, wit)[4]
    rng = SplitMix64(950 + n)
    rnd = [rng.below(R - 1) + 1 for _ in range(8)]
    dv, dy = rng.below(R - 1) + 1, rng.below(R - 1) + 1
    crs, buf = alloc_pinocchio(n, n_io, n_mid, max_degree)
    assert O.zkto_pinocchio_setup(ctypes.byref(crs), ptr(ints_to_arr(V, 4)), ptr(ints_to_arr(W, 4)), ptr(ints_to_arr(Y, 4)), ptr(ints_to_arr(rnd, 4))) == 0
    model = D.pinocchio_crs(V, W, Y, n, n_io, n_mid, max_degree, rnd)
    assert sorted(model) == sorted(buf) == sorted(D.PIN_GROUPS)
    for name, scalars in model.items():
        _same(buf[name], D.PIN_GROUPS[name], scalars, name)
    pf, pb = alloc_pinocchio_proof()
    for h_len in sorted({0, len(h)}):
        assert O.zkto_pinocchio_prove(ctypes.byref(crs), ptr(ints_to_arr(wit, 4)), ptr(ints_to_arr(h, 4)), h_len, ptr(fr(dv)), ptr(fr(dy)), ctypes.byref(pf)) == 0
        proof = D.pinocchio_proof(model, wit, h[:h_len], dv, dy, n_io)
        assert sorted(proof) == sorted(pb) == sorted(D.PIN_PROOF_GROUPS)
        for name, e in proof.items():
            _same(pb[name], D.PIN_PROOF_GROUPS[name], [e], (name, h_len))


def test_the_model_reduces_its_inputs():
    """values >= r give what their residues give, and the non-canonical inputs are what the GPU cases need: r + 1, 2^256 - 1, whole rows of such values"""
    rows, n, l = 5, 3, 2
    x = D.groth16_inputs(rows, n, l, 5, noncanonical=True)
    every = x["ui"] + x["vi"] + x["wi"] + x["trap"] + x["wires"] + x["h"] + [x["r"], x["s"]]
    assert all(R <= v < (1 << 256) for v in every) and {R + 1, D.TOP} <= set(x["trap"]) and {R + 1, D.TOP} <= set(x["ui"])
    assert set(x["ui"][:n]) <= set(D.NONCANONICAL) and set(x["wi"][-n:]) <= set(D.NONCANONICAL) and D.TOP in x["wires"] and D.TOP in x["h"]
    red = lambda v: [c % R for c in v]
    a = D.groth16_crs(x["ui"], x["vi"], x["wi"], n, l, rows - 1, *x["trap"])
    b = D.groth16_crs(red(x["ui"]), red(x["vi"]), red(x["wi"]), n, l, rows - 1, *red(x["trap"]))
    assert a == b
    assert D.groth16_proof(a, x["ui"], x["vi"], x["wires"], x["h"], x["r"], x["s"], n, l, rows - 1) == \
        D.groth16_proof(b, red(x["ui"]), red(x["vi"]), red(x["wires"]), red(x["h"]), x["r"] % R, x["s"] % R, n, l, rows - 1)
    p = D.pinocchio_inputs(2, 3, 3, 4, 6, noncanonical=True)
    every = p["vi"] + p["wi"] + p["yi"] + p["rnd"] + p["wires"] + p["h"] + [p["delta_v"], p["delta_y"]]
    assert all(R <= v < (1 << 256) for v in every) and {R + 1, D.TOP} <= set(p["rnd"])
    a = D.pinocchio_crs(p["vi"], p["wi"], p["yi"], 3, 2, 3, 4, p["rnd"])
    assert a == D.pinocchio_crs(red(p["vi"]), red(p["wi"]), red(p["yi"]), 3, 2, 3, 4, red(p["rnd"]))
    assert D.pinocchio_proof(a, p["wires"], p["h"], p["delta_v"], p["delta_y"], 2) == D.pinocchio_proof(a, red(p["wires"]), red(p["h"]), p["delta_v"] % R, p["delta_y"] % R, 2)
    with pytest.raises(AssertionError):
        D.groth16_crs(x["ui"], x["vi"], x["wi"], n, l, rows - 1, x["trap"][0], x["trap"][1], 2 * R, x["trap"][3], x["trap"][4])


def test_t_and_the_proof_follow_the_definitions():
    """t(x) against the product's coefficients, and the proof exponents against the verification equations (verifier.rs:30-54, pinocchio/verifier.rs:69-84) on a
    satisfied circuit: e(A, B) = e(alpha, beta) e(sum a_i uvw_i, gamma) e(C, delta) and v_s w_s = t h_s + y_s on the exponents"""
    t = [1]
    for i in range(1, 8): t = poly_mul(t, [(-i) % R, 1])
    assert D.t_at(12345, 7) == D.horner(t, 12345) and D.t_at(5, 7) == 0 and D.t_at(9, 0) == 1
    A, B, C, wit, l = chain_circuit(4)
    n, m = len(A), len(wit) - 1
    ui, vi, wi, h, _ = qap_from_r1cs(A, B, C, wit)
    U, V, W = flat(ui, n), flat(vi, n), flat(wi, n)
    x = D.groth16_inputs(m + 1, n, l, 21)
    crs = D.groth16_crs(U, V, W, n, l, m, *x["trap"])
    pf = D.groth16_proof(crs, U, V, wit, h, x["r"], x["s"], n, l, m)
    alpha, beta, gamma, delta = x["trap"][:4]
    stmt = sum(a * y for a, y in zip(wit[:l + 1], crs["g1_uvw_stmt"]))
    assert pf["A"] * pf["B"] % R == (alpha * beta + stmt * gamma + pf["C"] * delta) % R
    y = D.pinocchio_inputs(l + 1, m - l, n, n, 22)
    pc = D.pinocchio_crs(U, V, W, n, l + 1, m - l, n, y["rnd"])
    pp = D.pinocchio_proof(pc, wit, h, y["delta_v"], y["delta_y"], l + 1)
    io = lambda name: sum(a * e for a, e in zip(wit[:l + 1], pc[name]))
    assert (pp["v_mid_s"] + io("vk_io")) * (pp["g2_w_mid_s"] + io("wk_io")) % R == (pc["t"][0] * pp["h_s"] + pp["y_mid_s"] + io("yk_io")) % R
    assert pp["alpha_v_mid_s"] == pp["v_mid_s"] * pc["alpha_v"][0] % R and pp["alpha_w_mid_s"] == pp["g2_w_mid_s"] * pc["alpha_w"][0] % R
    assert pp["beta_vwy_mid_s"] * pc["gamma"][0] % R == (pp["v_mid_s"] + pp["g1_w_mid_s"] + pp["y_mid_s"]) * pc["beta_gamma"][0] % R


def test_model_constants_are_the_source_s():
    assert D.library_constants() == D.model_constants()


def test_gpu_cases_reach_every_cell():
    assert len(set(D.CELLS)) == len(D.CELLS)
    for case in D.all_cases():
        c = D.census(case)
        assert c and c <= set(D.CELLS), (D.case_id(case), c - set(D.CELLS))
    reached = D.gpu_case_census()
    assert not set(D.CELLS) - reached, sorted(set(D.CELLS) - reached)


def test_the_case_lists_are_the_ones_the_issue_names():
    assert D.G16_SHAPES == [(1, 1, 0), (63, 255, 0), (64, 256, 63), (65, 257, 3), (129, 2, 64)]
    assert D.PIN_SHAPES == [(0, 1, 1, 1), (2, 0, 2, 3), (1, 62, 2, 255), (12, 52, 5, 256), (13, 52, 4, 257), (0, 129, 2, 2)]
    assert D.VERIFY_IO == [0, 1, 12, 13, 20] and [k for k, _ in D.VERIFY_SEQUENCE] == [12, 2, 0, 12, 13, 2, 12]
    assert D.cache_walk(D.VERIFY_SEQUENCE, 12, 2) == ["build", "build", "none", "evict", "free", "hit", "rebuild"]
    for c in D.g16_cases():
        if not c["noncanonical"]: assert c["h_lens"] == sorted({0, 1, c["shape"][1]})
    for c in D.pin_cases():
        deg = c["shape"][3]
        assert {0, deg} <= set(c["h_lens"]) and {0, deg} <= set(c["resident_h_lens"]) and (deg < 2 or any(0 < v < deg for v in c["resident_h_lens"]))
    assert D.ORACLE_THREADS == 16


def test_a_changed_constant_breaks_the_census():
    """the cases are fixed; with other block widths or another PIN_FAST_IO some cell is left without a case"""
    k = D.model_constants()
    for name, value in [("LINCOMB_TPB", 128), ("LINCOMB_TPB", 512), ("POWSEQ_TPB", 128), ("PIN_FAST_IO", 11), ("PIN_FAST_IO", 16), ("PIN_TABLE_SLOTS", 4)]:
        assert set(D.CELLS) - D.gpu_case_census(dict(k, **{name: value})), (name, value)
    for value in (32, 128):
        assert set(D.CELLS) - D.gpu_case_census(dict(k, EVAL_ROWS_TPB=value, PIN_SCALARS_TPB=value, GENMUL_TPB=value)), value


def test_no_gpu_case_is_skipped_or_conditional():
    """every case list of the GPU module is the model's, whole, and nothing in the module skips.  A check of the module's TEXT: the census above counts the cases of
    dense_model, so it proves something about the GPU module only while that module runs exactly those lists."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_dense_protocols.py")) as f:
        text = f.read()
    hit = re.search(r"skip|xfail|importorskip", text)
    assert not hit, f"test_gpu_dense_protocols.py contains {hit.group(0)!r}: a case that may not run is not a case the census can count (the word is refused in comments too)"
    for pattern, what in [(r"parametrize\(\"case\", D\.g16_cases\(\), ids=D\.case_id\)", "the Groth16 test over D.g16_cases()"),
                          (r"parametrize\(\"case\", D\.pin_cases\(\), ids=D\.case_id\)", "the Pinocchio test over D.pin_cases()"),
                          (r"parametrize\(\"n_io\", D\.VERIFY_IO\)", "the verifier test over D.VERIFY_IO"),
                          (r"for n_io, key in D\.VERIFY_SEQUENCE", "the key sequence D.VERIFY_SEQUENCE"), (r"for z in D\.ZERO_MOD_R", "the zero trapdoors D.ZERO_MOD_R"),
                          (r"pytestmark = pytest\.mark\.gpu", "the module's gpu marker")]:
        assert re.search(pattern, text), f"test_gpu_dense_protocols.py no longer runs {what} as written here ({pattern}): if it was only reformatted, update this pattern"
    assert len(re.findall(r"parametrize\(", text)) == 3, "a parametrised test was added or removed: add its case list to dense_model.all_cases() and to this check"


@pytest.mark.parametrize("n_io", D.VERIFY_IO)
def test_chain_io_circuit_is_satisfied(n_io):
    A, B, C, wit = chain_io_circuit(n_io)
    assert len(wit) == len(A) + 2 >= max(D.VERIFY_IO) and wit[0] == 1
    V, W, Y, h, max_degree = pinocchio_instance(A, B, C, wit)          # asserts that t divides p
    assert len(h) <= max_degree and V.shape == (len(wit) * len(A), 4)


def test_the_oracle_refuses_trapdoors_that_are_zero_mod_r():
    """the oracle keeps step with zkt_groth16_setup / zkt_pinocchio_setup: status 1 (ZKT_ERR_INV_ZERO) and nothing written"""
    x = D.groth16_inputs(3, 2, 1, 31)
    U, V, W = (ints_to_arr(x[k], 4) for k in ("ui", "vi", "wi"))
    for pos in range(5):
        for z in D.ZERO_MOD_R:
            crs, buf = alloc_crs(2, 1, 2)
            for b in buf.values(): b[:] = 0xAB
            trap = list(x["trap"]); trap[pos] = z
            assert O.zkto_groth16_setup(ctypes.byref(crs), ptr(U), ptr(V), ptr(W), *[ptr(fr(t)) for t in trap]) == 1
            assert all((b == 0xAB).all() for b in buf.values())
    p = D.pinocchio_inputs(1, 2, 2, 2, 32)
    V, W, Y = (ints_to_arr(p[k], 4) for k in ("vi", "wi", "yi"))
    for pos in range(8):
        for z in D.ZERO_MOD_R:
            crs, buf = alloc_pinocchio(2, 1, 2, 2)
            for b in buf.values(): b[:] = 0xAB
            rnd = list(p["rnd"]); rnd[pos] = z
            assert O.zkto_pinocchio_setup(ctypes.byref(crs), ptr(V), ptr(W), ptr(Y), ptr(ints_to_arr(rnd, 4))) == 1
            assert all((b == 0xAB).all() for b in buf.values())
