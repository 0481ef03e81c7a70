"""Every plan and bucket-merge branch of the MSM (zk-toolkit_amd/csrc/zkt_msm_plan.cpp, msm_sort.h, zkt_msm.hip, msm_reduce_coop.h) against python integers, for G1, G2 and
secp256k1, resident (zkt_*_bases_from_device + zkt_*_msm_dev twice + submit/collect on two slots) and one-shot (zkt_*_msm).

The cases are built by tests/msm_plan_model.py, whose census of the scalars says which branch each case reaches — the hot-bucket boundary
(nt = 512 / 513), a full hot list (64) and a discarded one (65, and ~10 repeated random values), buckets of 8, 9, 16, 17, 64 and 65 pieces,
one point (or P and -P) in every term with one scalar, equal bucket sums, an infinite result, and n on both sides of every width, partition-sort
and graph step of both plans; tests/test_msm_plan_model.py checks those claims on the CPU.  Bases are k_i * G with known k_i, so the expected
sum is (sum k_i s_i mod order) * G, computed from python integers alone: neither the HIP path nor the oracle."""
import ctypes, importlib, os, subprocess, sys
import numpy as np
import pytest
import msm_plan_model as M
from zkt_testlib import G1W, G2W, G1_GEN, G2_GEN, SECP_GEN, py_g1_mul, py_g2_mul, py_secp_mul, g1_arr, g2_arr, secp_arr, to_abi_g2, ptr

pytestmark = pytest.mark.gpu
if os.environ.get("ZKT_MSM_C"):
    pytest.skip("a forced window width invalidates the census claims of these cases", allow_module_level=True)
zk = importlib.import_module("zk-toolkit_amd")

W = {"g1": G1W, "g2": G2W, "secp": 9}
GEN = {"g1": g1_arr([G1_GEN]), "g2": g2_arr([G2_GEN]), "secp": secp_arr([SECP_GEN])}


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


def _make_bases(L, group, ks):
    """k_i * G on the device (G1, G2) or through the host-pointer batch (secp256k1, which has no device form): (device tensor, host array)"""
    import torch
    n = len(ks)
    if group == "secp":
        host = np.zeros((n, 9), np.uint64)
        zk.check(L.zkt_secp_mul_batch(ptr(np.repeat(GEN["secp"], n, axis=0)), ptr(np.ascontiguousarray(ks)), 4, ptr(host), n))
        return torch.from_numpy(host.view(np.int64)).cuda(), host
    d_gen = torch.from_numpy(np.repeat(GEN[group], n, axis=0).view(np.int64)).cuda()
    d_k = torch.from_numpy(np.ascontiguousarray(ks).view(np.int64)).cuda()
    d_out = torch.empty((n, W[group]), dtype=torch.int64, device="cuda")
    zk.check(getattr(L, f"zkt_{group}_mul_batch_dev")(_vp(d_gen), _vp(d_k), 4, _vp(d_out), n, None))
    torch.cuda.synchronize()
    return d_out, d_out.cpu().numpy().view(np.uint64)


_shared = {}


def _bases_for(L, case):
    """the case's bases: a prefix of the group's shared random set, or built for the case (same point, P and -P)"""
    if case.kspec[0] == "random":
        key = (case.group, case.kspec)
        if key not in _shared:
            ks = M.random_ks(case.kspec[1])
            _shared[key] = _make_bases(L, case.group, ks) + (M.ints_from_scalars(ks),)
        d, host, kint = _shared[key]
        return d[: case.n], host[: case.n], kint[: case.n]
    ks = case.ks()
    return _make_bases(L, case.group, ks) + (M.ints_from_scalars(ks),)


def _resident(L, group, d_bases, n, scalars):
    """msm_dev twice (below 2^19 terms: the graph is captured, then replayed) and one submit/collect over two slots: all four results must agree"""
    import torch
    h = ctypes.c_void_p()
    zk.check(getattr(L, f"zkt_{group}_bases_from_device")(_vp(d_bases), n, None, ctypes.byref(h)))
    try:
        d_s = torch.from_numpy(np.ascontiguousarray(scalars).view(np.int64)).cuda()
        outs = []
        for _ in range(2):
            got = np.zeros((1, W[group]), np.uint64)
            zk.check(getattr(L, f"zkt_{group}_msm_dev")(h, _vp(d_s), n, None, ptr(got), None))
            outs.append(got)
        for slot in (0, 1):
            zk.check(getattr(L, f"zkt_{group}_msm_submit")(h, _vp(d_s), n, None, slot))
        for slot in (0, 1):
            got = np.zeros((1, W[group]), np.uint64)
            zk.check(getattr(L, f"zkt_{group}_msm_collect")(h, slot, ptr(got), None))
            outs.append(got)
        return outs
    finally:
        getattr(L, f"zkt_{group}_bases_free")(h)


def _oneshot(L, group, host_bases, n, scalars):
    got = np.zeros((1, W[group]), np.uint64)
    zk.check(getattr(L, f"zkt_{group}_msm")(ptr(np.ascontiguousarray(host_bases)), ptr(np.ascontiguousarray(scalars)), n, ptr(got)))
    return [got]


def _run(L, case):
    d_bases, host_bases, kint = _bases_for(L, case)
    tot = sum(k * s for k, s in zip(kint, M.ints_from_scalars(case.scalars))) % M.ORDER[case.group]
    want = _point(case.group, tot)
    outs = _resident(L, case.group, d_bases, case.n, case.scalars) if case.form == "resident" else _oneshot(L, case.group, host_bases, case.n, case.scalars)
    for i, got in enumerate(outs):
        assert (got == want).all(), f"{case.group} {case.form} {case.name}: result {i} (msm_dev, msm_dev replayed, slot 0, slot 1) differs from python integers"


_BRANCH = [(g, f, cid) for g in M.GROUPS for f in M.FORMS for cid, _ in M.cases(g, f)]


@pytest.mark.parametrize("group,form,cid", _BRANCH, ids=[f"{g}-{f}-{c}" for g, f, c in _BRANCH])
def test_msm_branch_case(L, group, form, cid):
    case = dict(M.cases(group, form))[cid]()
    assert not M.check_claim(case)
    _run(L, case)


_STEPS = [(g, f, n) for g in M.GROUPS for f in M.FORMS for n in M.plan_steps(f)]


@pytest.mark.parametrize("group,form,n", _STEPS, ids=[f"{g}-{f}-n{n}" for g, f, n in _STEPS])
def test_msm_plan_step(L, group, form, n):
    _run(L, M.case_plan_step(group, form, n))


def test_msm_plans_with_poisoned_workspaces():
    """This module again in a child process with ZKT_DEBUG_POISON=1: every MSM workspace starts as 0xA5 bytes, so a branch that reads a word
    nobody wrote (hot_part, partial, the task list of a discarded hot list, a cancelled bucket) fails instead of reading a fresh allocation's zeros."""
    if os.environ.get("ZKT_DEBUG_POISON"):
        pytest.skip("already inside the poisoned child")
    here = os.path.abspath(__file__)
    env = dict(os.environ, ZKT_DEBUG_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
