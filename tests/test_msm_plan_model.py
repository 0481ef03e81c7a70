"""CPU checks of the MSM plan model (tests/msm_plan_model.py): its signed digits reconstruct every scalar exactly, its plan is pinned to the
library's own workspace size (so a retuned plan table fails here, on any machine), and every case of tests/test_gpu_msm_plans.py reaches the
branch it claims — checked before anything runs on a GPU."""
import importlib, os
import numpy as np
import pytest
import msm_plan_model as M

R = M.R_ORDER
EDGES = [0, 1, R - 1, R, 1 << 255, (1 << 256) - 1, M.SECP_ORDER - 1, (1 << 254) + 12345]


def _edge_scalars(c):
    """the fixed edges plus, for width c, a window equal to half (positive, no carry), half + 1 (negative), and a run of all-ones windows that receives a carry"""
    half = 1 << (c - 1)
    xs = list(EDGES)
    xs.append(half << c)                                              # window 1 = half exactly
    xs.append((half + 1) << (2 * c))                                  # window 2 = half + 1: negative digit, carry into window 3
    ones = (1 << c) - 1
    xs.append((ones << c) | (half + 1))                               # window 0 negative, window 1 all ones: raw 2^c after the carry
    xs.append(((1 << (c * (256 // c))) - 1) & ((1 << 256) - 1))       # every full window all ones
    return [x & ((1 << 256) - 1) for x in xs]


@pytest.mark.parametrize("c", range(4, 21))
def test_digits_reconstruct_the_scalar(c):
    nwin = (256 + c) // c
    rng = np.random.Generator(np.random.PCG64(100 + c))
    rnd = rng.integers(0, 2**64, size=(300, 4), dtype=np.uint64)
    xs = _edge_scalars(c) + M.ints_from_scalars(rnd)
    mag, neg = M.digits(M.scalars_from_ints(xs), c, nwin)
    assert (mag >= 0).all() and (mag <= 1 << (c - 1)).all()
    assert not neg[-1].any(), "the top window never carries out"
    for i, x in enumerate(xs):
        back = sum((-1 if neg[w, i] else 1) * int(mag[w, i]) << (c * w) for w in range(nwin))
        assert back == x, (c, hex(x))


def test_bucket_ids_skip_zero_digits_and_infinity_bases():
    s = M.scalars_from_ints([0, 1, 5 << 13, 1])
    b = M.bucket_ids(s, np.array([0, 0, 0, 1], bool), 13, 20, "oneshot")
    assert (b[:, 0] == -1).all() and (b[:, 3] == -1).all()
    assert b[0, 1] == 0 and (b[1:, 1] == -1).all()
    assert b[1, 2] == 4096 + 4 and b[0, 2] == -1
    assert M.bucket_ids(s, None, 13, 20, "resident")[1, 2] == 4


PIN_N = (1, 1023, 1024, 2047, 2048, 16383, 16384, 246723, 246724, (1 << 19) - 1, 1 << 19, 1 << 20)


@pytest.mark.skipif(bool(os.environ.get("ZKT_MSM_C")), reason="the library reads the width override once per process: the pinned plan is the default one")
def test_model_is_pinned_to_the_library_workspace_size():
    zk = importlib.import_module("zk-toolkit_amd")
    L = zk.lib()
    for n in PIN_N:
        assert L.zkt_g1_msm_workspace_bytes(n) == M.g1_resident_workspace_bytes(n), n


GROUP_ID = {"g1": 0, "g2": 1, "secp": 2}                  # zkt_internal.h, GroupId
CARVE_PTRS = 27                                           # hostcheck.cpp, zkt_hostcheck_msm_carve: the first six are used at 256-byte alignment, the rest as words
CARVE_ALIGN = (256,) * 6 + (4,) * (CARVE_PTRS - 6)


def test_the_carve_ends_inside_the_workspace_of_every_plan():
    """The plans sum their ws_bytes by hand (zkt_msm_plan.cpp: msm_plan, msm_plan_direct) while carve() hands the workspace out: in the host build of that file, the
    carve's end lies inside ws_bytes and every pointer is aligned for its use, for all groups and forms; and the model restates ws_bytes for every group, not G1 only."""
    import ctypes
    H = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zk-toolkit_amd", "libzkt_hostcheck.so"))
    H.zkt_hostcheck_msm_ws_bytes.restype = H.zkt_hostcheck_msm_carve.restype = ctypes.c_size_t
    H.zkt_hostcheck_msm_ws_bytes.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    H.zkt_hostcheck_msm_carve.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    offs = (ctypes.c_size_t * CARVE_PTRS)()
    null = ctypes.c_size_t(-1).value
    sizes = sorted(set(M.RESIDENT_STEPS) | set(M.ONESHOT_STEPS) | set(PIN_N) | {1, 2, 3, (1 << 20) + 1, 1 << 22})
    runs = [(form, n, 0) for form in (0, 1) for n in sizes] + [(2, n, k) for n in (1, 1024, 16384, 1 << 17) for k in (1, 2, 31, 32)]
    default_widths = not os.environ.get("ZKT_MSM_C")      # the library reads the width override once per process; the model restates the default plan
    least = {}
    for group in M.GROUPS:
        for form, n, k in runs:
            ws = H.zkt_hostcheck_msm_ws_bytes(n, GROUP_ID[group], form, k)
            end = H.zkt_hostcheck_msm_carve(n, GROUP_ID[group], form, k, offs)
            assert end <= ws, (group, form, n, k, end, ws)
            for i, (o, a) in enumerate(zip(offs, CARVE_ALIGN)):
                assert o == null or (o % a == 0 and o < end), (group, form, n, k, i, o)
            assert all(o != null for o in offs[:4]) and (offs[4] == null) == (form == 2), (group, form, n, k)
            if form == 1 or (form == 0 and default_widths):      # (msm_plan_direct does not read the override)
                assert ws == M.plan(n, group, M.FORMS[form])["ws_bytes"], (group, form, n)
            if form not in least or ws - end < least[form][0]:
                least[form] = (ws - end, ("resident", "direct", "batch")[form], group, n, k)
    for slack in least.values():      # (the batched plan takes its size from the carve plus 4096: its slack is that constant)
        print("smallest slack between the carve's end and ws_bytes: %d bytes (%s form, %s, n = %d, k = %d)" % slack)


def test_plan_steps_cover_every_combination_the_plan_can_pick():
    for form in M.FORMS:
        cand = {1}
        for k in range(1, 20):
            cand |= {(1 << k) - 1, 1 << k}
        for c in range(4, 21):
            nwin = (256 + c) // c
            t = (M.PART_MIN_ENTRIES + nwin - 1) // nwin
            cand |= {t - 1, t}
        cand = {n for n in cand if 1 <= n <= M.PLAN_N_MAX}
        combo = lambda n: (M.plan(n, "g1", form)["c"], M.plan(n, "g1", form)["partition"], M.plan(n, "g1", form)["graph"])
        want = {combo(n) for n in cand}
        got = {combo(n) for n in M.plan_steps(form)}
        assert got == want, (form, want - got)
        # every step really is a step: each pair (n - 1, n) of the list differs in width, sort or graph
        steps = M.plan_steps(form)
        for lo, hi in zip(steps[::2], steps[1::2]):
            assert hi == lo + 1 and combo(lo) != combo(hi), (form, lo)
    assert M.plan(246724, "g1", "resident")["partition"] and not M.plan(246723, "g1", "resident")["partition"]
    assert M.plan(220753, "g2", "oneshot")["partition"] and not M.plan(220752, "secp", "oneshot")["partition"]


@pytest.mark.parametrize("form", M.FORMS)
@pytest.mark.parametrize("group", M.GROUPS)
def test_every_gpu_case_reaches_its_branch(group, form):
    for cid, build in M.cases(group, form):
        case = build()
        assert len(case.scalars) == case.n and len(case.ks()) == case.n
        bad = M.check_claim(case)
        assert not bad, (group, form, cid, bad)
    # the step list: its sizes give the plan they are listed for, and the edge scalars are in place
    for n in M.plan_steps(form):
        case = M.case_plan_step(group, form, n)
        assert case.scalars.shape == (n, 4) and M.ints_from_scalars(case.scalars[-1:]) == [(1 << 256) - 1]


def test_the_cases_together_reach_every_merge_branch():
    """over all cases of one prime-field group and one form: single, group, block (lane / block scatter), bulk, listed hot, discarded list"""
    for form in M.FORMS:
        seen = dict(single=0, group=0, block_lane_scatter=0, block_scatter=0, bulk=0, hot_listed=0, overflow=0)
        for _, build in M.cases("g1", form):
            cen = build().census()
            for k in ("single", "group", "block_lane_scatter", "block_scatter", "bulk"):
                seen[k] += cen[k]
            seen["hot_listed"] += cen["hot"] if not cen["overflow"] else 0
            seen["overflow"] += cen["overflow"]
        assert all(v > 0 for v in seen.values()), (form, seen)
