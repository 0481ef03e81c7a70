"""Pinocchio verification against a resident key: zkt_pinocchio_vk_create once (timed on its own), then zkt_pinocchio_verify_batch on n copies of one honest proof, and a
loop of single zkt_pinocchio_verify calls as the baseline.  profiles/pinocchio_verify_batch_timing.md holds the rows.

  python tools/bench_pinocchio_verify.py                          every batch size, then 64 single calls
  python tools/bench_pinocchio_verify.py --sizes 1024,2048,4096   the sizes of the switch-over measurement; run it once with ZKT_DPRODUCT_MAX=1000000 (every size on the
                                                                  lane-distributed kernels) and once with ZKT_DPRODUCT_MAX=0 (every size on k_pinocchio_check)
  python tools/bench_pinocchio_verify.py --baseline-lib <libzkt_hip.so of another build>      the single-call loop alone on that build, loaded with plain ctypes
                                                                  (a build from before zkt_pinocchio_vk_create lacks symbols the package asks for)"""
import argparse, ctypes, importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from zkt_testlib import *
from qap_util import *

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1,16,256,1024,2048,4096,65536")
ap.add_argument("--singles", type=int, default=64)
ap.add_argument("--constraints", type=int, default=8, help="chain circuit size (the verifier's work does not depend on it: n_io = 2)")
ap.add_argument("--baseline-lib", default=None)
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",") if s] if not args.baseline_lib else []

zk = importlib.import_module("zk-toolkit_amd")
if args.baseline_lib:
    import torch  # noqa: F401  (one HIP runtime per process, as zk.lib() arranges)
    L = ctypes.CDLL(os.path.abspath(args.baseline_lib)); lib_name = args.baseline_lib
    L.zkt_pinocchio_prove.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    assert L.zkt_init(-1) == 0
else:
    zk.init(); L = zk.lib(); lib_name = os.path.relpath(zk.LIB_PATH, ROOT)
def check(rc):
    if rc != 0: raise RuntimeError("zkt status %d" % rc)
A, B, C, wit, l = chain_circuit(args.constraints)
n_c, n_io = len(A), l + 1
V, W, Y, h, max_degree = pinocchio_instance(A, B, C, wit)
rng = SplitMix64(4096)
rnd = ints_to_arr([rng.below(R - 1) + 1 for _ in range(8)], 4)
dv, dy = ints_to_arr([rng.below(R - 1) + 1], 4), ints_to_arr([rng.below(R - 1) + 1], 4)
wires, H = ints_to_arr(wit, 4), ints_to_arr(h, 4)
crs, cbuf = alloc_pinocchio(n_c, n_io, len(wit) - n_io, max_degree)
check(L.zkt_pinocchio_setup(ctypes.byref(crs), ptr(V), ptr(W), ptr(Y), ptr(rnd)))
pf, pb = alloc_pinocchio_proof()
check(L.zkt_pinocchio_prove(ctypes.byref(crs), ptr(wires), ptr(H), len(h), ptr(dv), ptr(dy), ctypes.byref(pf)))
io = wires[:n_io].copy()
limit = os.environ.get("ZKT_DPRODUCT_MAX", "default")

if sizes:
    vk = ctypes.c_void_p()
    t0 = time.perf_counter(); check(L.zkt_pinocchio_vk_create(ctypes.byref(crs), ctypes.byref(vk))); t_key = (time.perf_counter() - t0) * 1e3
    print("zkt_pinocchio_vk_create  n_io=%d  %.2f ms" % (n_io, t_key))
    for n in sizes:
        bufs = {k: np.repeat(v, n, axis=0) for k, v in pb.items()}
        bp = PinProof()
        for k, v in bufs.items(): setattr(bp, k, ptr(v))
        ios = np.tile(io, (n, 1)); verdict = np.zeros(n, np.int32)
        call = lambda: check(L.zkt_pinocchio_verify_batch(vk, ctypes.byref(bp), ptr(ios), n, verdict.ctypes.data_as(ctypes.c_void_p)))
        call()                                               # the first call of a size pays the pool's growth
        ts = []
        for _ in range(3 if n <= 4096 else 2):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
        dt = min(ts)
        print("pinocchio verify_batch  proofs=%6d  %9.2f ms  %9.0f/s  all accepted=%s  (ZKT_DPRODUCT_MAX=%s)" % (n, dt * 1e3, n / dt, bool((verdict == 1).all()), limit), flush=True)
    L.zkt_pinocchio_vk_free(vk)
if args.singles:
    assert L.zkt_pinocchio_verify(ctypes.byref(crs), ctypes.byref(pf), ptr(io)) == 1       # first sight of the key: its tables are built here
    t0 = time.perf_counter()
    for _ in range(args.singles): assert L.zkt_pinocchio_verify(ctypes.byref(crs), ctypes.byref(pf), ptr(io)) == 1
    dt = (time.perf_counter() - t0) / args.singles
    print("pinocchio verify, %d single calls  %.3f ms per proof  %.0f/s  (library %s)" % (args.singles, dt * 1e3, 1 / dt, lib_name))
