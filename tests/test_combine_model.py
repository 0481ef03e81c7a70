"""CPU checks of tests/combine_model.py: every case of the combine reaches the (site, class) cells it claims, the cases together cover the table the
issue of an untested jac_add exit would hide in, the loop condition and the tree guard sit on both sides of their edges, and the lines of
zk-toolkit_amd/csrc the model restates still read as it restates them."""
import pytest
import combine_model as C


def test_the_model_sums_and_classifies():
    order = 101
    r = C.Run([5, None, 96, 7], order)              # lanes 0..3; level2: 5 + 96 = opposite, None + 7 = inf+x; level1: inf + 7
    assert r.total == 7
    assert [(s, c) for s, c, _ in r.additions] == [("loop", "inf+x"), ("loop", "inf+inf"), ("loop", "inf+x"), ("loop", "inf+x"),
                                                   ("level2", "opposite"), ("level2", "inf+x"), ("level1", "inf+x")]
    r = C.Run([3] * 65 + [4], order)                # lanes 0 and 1 read twice
    assert r.total == (3 * 65 + 4) % order
    assert ("loop", "equal", 0) in r.additions and ("loop", "generic", 1) in r.additions
    assert C.Run([None], order).total is None and C.Run([50, 51], order).total is None


@pytest.mark.parametrize("group", C.GROUPS)
def test_every_claim_holds(group):
    for case in C.CASES:
        assert C.check_claim(case, group) == []
        assert case.claim, case.name
        parts = case.parts(group)
        want = sum(c for c in parts if c is not None) % C.ORDER[group] or None
        assert case.run(group).total == want, case.name


def test_the_census_is_the_same_in_every_group():
    for case in C.CASES:
        assert C.census(case, "g1") == C.census(case, "g2") == C.census(case, "secp"), case.name


def test_a_false_claim_is_noticed():
    case = C.Case("wrong", ["P", "inf0", "P"], {("level1", "equal")})       # they meet at level 2
    assert C.check_claim(case) and ("level2", "equal") in C.census(case)


def test_the_cases_cover_the_table():
    u = C.union_census()
    missing = [(s, c) for s in C.SITES for c in ("equal", "opposite", "inf+x", "x+inf", "generic", "inf+inf") if (s, c) not in u]
    assert missing == []


def test_the_case_list_is_the_announced_one():
    names = [c.name for c in C.CASES]
    assert [n for n in names if n.startswith("distinct-")] == [f"distinct-{n}" for n in C.DISTINCT_COUNTS]
    assert C.DISTINCT_COUNTS == (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
    for a, b in ((0, 64), (0, 32), (0, 16), (0, 8), (0, 4), (0, 2), (0, 1), (63, 127), (31, 63)):
        count = max(a, b) + 1
        for v in ("same", "prime", "opposite"):
            assert f"pair-{a}-{b}-n{count}-{v}" in C.CASE
            q = C.third_position(a, b)
            assert (q is None) == ((a, b) == (0, 1))            # the one pair whose meeting is the kernel's last addition: nothing can join afterwards
            if q is not None:
                withq = C.CASE[f"pair-{a}-{b}-n{count}-{v}-q{q}"]
                assert withq.count == count and withq.tokens.count("Q") == 1
                assert withq.run().total not in (None, 2 * C.logs("g1")["P"] % C.ORDER["g1"])
    assert all(f"all-inf-{n}" in C.CASE for n in (1, 2, 65)) and all(f"all-equal-{n}" in C.CASE for n in (8, 64))
    for n in (8, 64):
        r = C.CASE[f"all-equal-{n}"].run()
        assert {c for s, c, _ in r.additions if s != "loop"} == {"equal"} and r.total == n * C.logs("g1")["P"] % C.ORDER["g1"]
    lg = C.logs("g1")
    gen = [lg[("g", i)] for i in range(C.GENERIC_N)]
    assert len(set(gen)) == C.GENERIC_N and all(c & 1 for c in gen)
    both = {t for c in C.CASES for t in c.tokens if t in C.INF_TOKENS}
    assert both == set(C.INF_TOKENS)                        # both constructions of infinity are operands


def test_the_guards_sit_on_both_sides_of_their_edges():
    for count in (32, 33, 63, 64, 65, 128, 129):
        assert f"distinct-{count}" in C.CASE
        g = C.guard_sides(count)
        assert g["loop"] == (True, True), count             # partial count - 1 is read, index count (the poisoned guard partial of the GPU test) is refused
        if count < C.LANES:
            assert g["tree"] == (True, True), count         # lane pair ending at count - 1 admitted, the pair ending at count refused
        else:
            assert not g["tree"][1] and all(ok for _, _, ok in C.Run([1] * count, 1 << 61).tree_guard), count
    # 32 | 33: lane 0 of level 32; 63 | 64: lane 31 of level 32; 64 | 65 and 128 | 129: lane 0's second and third pass
    assert (32, 0, False) in C.Run([1] * 32, 1 << 61).tree_guard and (32, 0, True) in C.Run([1] * 33, 1 << 61).tree_guard
    assert (32, 31, False) in C.Run([1] * 63, 1 << 61).tree_guard and (32, 31, True) in C.Run([1] * 64, 1 << 61).tree_guard
    assert (0, 64, False) in C.Run([1] * 64, 1 << 61).loop_guard and (0, 64, True) in C.Run([1] * 65, 1 << 61).loop_guard
    assert (0, 128, False) in C.Run([1] * 128, 1 << 61).loop_guard and (0, 128, True) in C.Run([1] * 129, 1 << 61).loop_guard


def test_the_model_restates_the_source():
    for what, want, found in C.source_line_counts():
        assert found == want, f"{what}: the line the model restates occurs {found} times in the source, expected {want}"
