"""CPU checks of tests/poly_model.py: its Kronecker product equals the reference's schoolbook loop, its divrem equals the reference's long division,
its plan constants are the ones csrc/zkt_poly.hip and include/zkt.h hold, and the case lists of tests/test_gpu_poly.py reach every cell of the plan —
checked before anything runs on a GPU."""
import random
import pytest
import poly_model as P

R = P.R


def _poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def test_kronecker_equals_schoolbook_on_random_shapes():
    rng = random.Random(1)
    shapes = [(1, 1), (70, 33), (33, 70), (1, 70)] + [(rng.randrange(1, 71), rng.randrange(1, 34)) for _ in range(16)]
    assert len(shapes) == 20
    for na, nb in shapes:
        a, b = _poly(rng, na), _poly(rng, nb)
        assert P.kron_mul(a, b) == P.school_mul(a, b), (na, nb)


def test_kronecker_reduces_its_inputs_and_takes_extreme_coefficients():
    a = [R - 1] * 40; b = [R - 1] * 40
    assert P.kron_mul(a, b) == P.school_mul(a, b)
    assert P.kron_mul([R, R + 1, (1 << 256) - 1], [5]) == [0, 5, ((1 << 256) - 1) % R * 5 % R]


def test_zero_operand_keeps_its_length():
    """multiply_by does not normalise: a zero operand gives na + nb - 1 zeros (polynomial.rs:173-190)"""
    assert P.kron_mul([0, 0, 0], [1, 2]) == [0] * 4 == P.school_mul([0, 0, 0], [1, 2])
    assert P.kron_mul([0], [7]) == [0]


def test_divrem_equals_long_division():
    rng = random.Random(2)
    for L, nb in [(1, 1), (1, 7), (7, 1), (20, 33), (33, 20), (64, 2), (50, 50)]:
        b = _poly(rng, nb); b[-1] = rng.randrange(1, R)
        a = _poly(rng, L + nb - 1)
        q, rem = P.divrem(a, b)
        assert (q, rem) == P.long_division(a, b), (L, nb)
        assert len(q) == L and len(rem) <= nb - 1
        back = P.school_mul(q, b)
        assert [(x + (rem[i] if i < len(rem) else 0)) % R for i, x in enumerate(back)] == a


def test_divrem_exact_zero_leading_and_non_monic():
    rng = random.Random(3)
    q, b = _poly(rng, 9), _poly(rng, 5)
    b[-1] = 12345
    a = P.school_mul(q, b)
    assert P.divrem(a, b) == (q, [])                                  # DivResult::Quotient
    assert P.divrem(a + [0, 0], b) == (q + [0, 0], [])                # zero leading coefficients of a: q is zero-padded
    rem = [7, 0, 0, 0]                                                # a remainder with zero high coefficients
    a2 = [(x + (rem[i] if i < 4 else 0)) % R for i, x in enumerate(a)]
    assert P.divrem(a2, b) == (q, [7]) == P.long_division(a2, b)


def test_tree_t_equals_the_running_product():
    for n in (0, 1, 2, 3, 7, 64, 65, 100):
        t = [1]
        for i in range(1, n + 1): t = P.school_mul(t, [(-i) % R, 1])
        assert P.tree_t(n) == t, n
    t = P.tree_t(1000)
    assert len(t) == 1001 and t[-1] == 1 and all(P.horner(t, x) == 0 for x in (1, 500, 1000)) and P.horner(t, 1001) != 0


def test_shifted_sum_is_a_sparse_product():
    rng = random.Random(4)
    b = _poly(rng, 10)
    a = [0] * 9; a[0], a[1], a[8] = 3, 5, 9
    assert P.shifted_sum([(0, 3), (1, 5), (8, 9)], b, 18) == P.school_mul(a, b)


def test_model_constants_are_the_source_s():
    assert P.library_constants() == P.model_constants()


def test_transform_launch_groups():
    assert [P.ntt_launches(k) for k in (1, 10, 11, 18, 19, 21)] == [1, 1, 2, 2, 3, 3]
    assert P.mul_plan(512, 513, D=64) == {"path": "ntt", "logN": 10, "launches": 1, "transforms": 3, "square": False}
    assert P.mul_plan(513, 513, D=64)["logN"] == 11 and P.mul_plan(513, 513, D=64)["launches"] == 2
    assert P.mul_plan(*P.BIG_MUL, D=64)["logN"] == 19 and P.mul_plan(*P.BIG_MUL, D=64)["launches"] == 3
    assert P.mul_plan(*P.LIMIT_MUL, D=64)["logN"] == 21


def test_newton_steps_and_division_plans():
    assert P.newton_steps(1) == [] and P.newton_steps(2) == [2] and P.newton_steps(65) == [2, 4, 8, 16, 32, 64, 128]
    assert P.newton_steps(1 << 17) == [1 << k for k in range(1, 18)]
    assert P.div_plan(64 + 32, 33, D=64, Dd=64)["quotient"] == "direct" and P.div_plan(65 + 32, 33, D=64, Dd=64)["quotient"] == "newton"
    p = P.div_plan(1025 + 999, 1000, D=64, Dd=64)
    assert p["rem"] == "fold" and p["rem_logN"] == 10 and p["steps"][-1] == 2048
    assert P.div_plan(4097 + 1, 2, D=64, Dd=64)["rem"] == "direct" and P.div_plan(7, 1, D=64, Dd=64)["rem"] == "none"


def test_tree_levels():
    assert P.tree_levels(1) == [] and P.tree_levels(2) == [(1, 1, "direct", False, True)]
    lv = P.tree_levels(1000, D=64)
    assert [l[0] for l in lv] == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    assert [l[2] for l in lv] == ["direct"] * 7 + ["ntt"] * 3
    assert lv[3] == (8, 63, "direct", True, True)                      # 125 children of 8 roots: the last node has one child
    assert P.tree_levels(4096, D=64)[-1] == (2048, 1, "ntt", False, True)


def test_evaluation_plan():
    assert P.eval_plan(1000, 1000) == "horner" and P.eval_plan(1 << 20, 1) == "split" and P.eval_plan(1 << 20, 1024) == "horner"
    assert P.eval_plan(P.EVAL_SPLIT_MIN_N - 1, 1) == "horner" and P.eval_plan(P.EVAL_SPLIT_MIN_N, 1) == "split"


def test_gpu_cases_reach_every_cell():
    reached = P.gpu_case_census()
    assert reached <= set(P.CELLS), reached - set(P.CELLS)
    assert not set(P.CELLS) - reached, sorted(set(P.CELLS) - reached)


@pytest.mark.parametrize("D,Dd", [(16, 16), (64, 64), (256, 128), (1024, 512)])
def test_both_sides_of_both_thresholds_are_cases_whatever_the_thresholds(D, Dd):
    """the case lists follow the source's constants: with any threshold, D and D + 1 (Dd and Dd + 1) land on opposite paths"""
    assert P.census_mul(D, D, D=D) >= {"mul_direct", "mul_direct_edge"} and "mul_ntt_edge" in P.census_mul(D + 1, D + 1, D=D)
    assert P.census_mul(D, 3000, D=D) >= {"mul_direct_edge"} and "mul_ntt_edge" in P.census_mul(3000, D + 1, D=D)
    assert "div_direct_edge" in P.census_div(Dd + 32, 33, D, Dd) and "div_newton_edge" in P.census_div(Dd + 33, 33, D, Dd)
