#!/usr/bin/env python3
"""Batched MSM against the slot ring: k scalar vectors over one resident base set, once as ONE zkt_*_msm_batch_dev call and once as k zkt_*_msm_submit
calls plus k collects on the same handle (slots 0..7, at most eight in flight).  Both paths are warmed (every slot the ring uses, the batch with the largest
k), then alternated; a host clock runs around calls that end in the collect.  Prints one markdown table row per (group, n, k): median / min / max of both
paths in ms, the ring's median over the even against the odd repeats (its spread against itself), and whether all 2k results agree bit for bit.
usage: msm_batch_timing.py --group g1|g2|secp --n N [--ks 2,5,16] [--reps 30] [--out FILE.md]"""
import argparse, ctypes, importlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import msm_plan_model as M
from zkt_testlib import G1W, G2W, G1_GEN, G2_GEN, SECP_GEN, g1_arr, g2_arr, secp_arr, ptr

ap = argparse.ArgumentParser()
ap.add_argument("--group", required=True, choices=("g1", "g2", "secp")); ap.add_argument("--n", type=int, required=True)
ap.add_argument("--ks", default="2,5,16"); ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
a = ap.parse_args()
grp, n, ks, reps = a.group, a.n, [int(x) for x in a.ks.split(",")], a.reps
zk = importlib.import_module("zk-toolkit_amd"); zk.init(0); L = zk.lib()
W = {"g1": G1W, "g2": G2W, "secp": 9}[grp]
gen = {"g1": g1_arr([G1_GEN]), "g2": g2_arr([G2_GEN]), "secp": secp_arr([SECP_GEN])}[grp]
vp = lambda t: ctypes.c_void_p(t.data_ptr())
fn = lambda name: getattr(L, f"zkt_{grp}_{name}")

# bases k_i * G
kb = np.ascontiguousarray(M.random_ks(M.K_SEED)[:n])
if grp == "secp":
    host = np.zeros((n, 9), np.uint64)
    zk.check(L.zkt_secp_mul_batch(ptr(np.repeat(gen, n, axis=0)), ptr(kb), 4, ptr(host), n))
    d_b = torch.from_numpy(host.view(np.int64)).cuda()
else:
    d_g = torch.from_numpy(np.repeat(gen, n, axis=0).view(np.int64)).cuda(); d_k = torch.from_numpy(kb.view(np.int64)).cuda()
    d_b = torch.empty((n, W), dtype=torch.int64, device="cuda")
    zk.check(fn("mul_batch_dev")(vp(d_g), vp(d_k), 4, vp(d_b), n, None)); torch.cuda.synchronize()
h = ctypes.c_void_p(); zk.check(fn("bases_from_device")(vp(d_b), n, None, ctypes.byref(h)))

kmax = max(ks)
rng = np.random.Generator(np.random.PCG64(9))
s = rng.integers(0, 2**64, size=(kmax * n, 4), dtype=np.uint64); s[:, 3] >>= np.uint64(2)          # k distinct vectors of 254-bit scalars, vec_stride = n
d_s = torch.from_numpy(s.view(np.int64)).cuda()
vec = lambda v: ctypes.c_void_p(d_s.data_ptr() + v * n * 32)
SLOTS = 8


def ring_run(k, out):
    """k submits and k collects, at most SLOTS in flight; ends with the last collect"""
    sub = col = 0
    while col < k:
        while sub < k and sub - col < SLOTS:
            zk.check(fn("msm_submit")(h, vec(sub), n, None, sub % SLOTS)); sub += 1
        zk.check(fn("msm_collect")(h, col % SLOTS, ptr(out[col: col + 1]), None)); col += 1


def batch_run(k, out):
    zk.check(fn("msm_batch_dev")(h, vp(d_s), n, k, n, None, ptr(out), None))


o_ring, o_batch = np.zeros((kmax, W), np.uint64), np.zeros((kmax, W), np.uint64)
for _ in range(3): ring_run(min(kmax, 2 * SLOTS), o_ring)              # every slot the ring uses, graphs captured
for _ in range(3): batch_run(kmax, o_batch)                            # the batch with the largest k: nothing is allocated afterwards
lines = []
for k in ks:
    for _ in range(2): ring_run(k, o_ring); batch_run(k, o_batch)
    tr, tb = [], []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); ring_run(k, o_ring); tr.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize(); t0 = time.perf_counter(); batch_run(k, o_batch); tb.append((time.perf_counter() - t0) * 1e3)
    same = bool((o_ring[:k] == o_batch[:k]).all())
    med = statistics.median
    line = "| %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f / %.3f | %.2f | %s |" % (
        grp, n, k, med(tr), min(tr), max(tr), med(tb), min(tb), max(tb), med(tr[0::2]), med(tr[1::2]), med(tr) / med(tb), "yes" if same else "NO")
    print(line, flush=True); lines.append(line)
fn("bases_free")(h)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if all(l.endswith("yes |") for l in lines) else 1)
