#!/usr/bin/env python3
"""Where the dense Fr polynomial engine (csrc/zkt_poly.hip) should switch from its direct kernels to the transform paths.

  poly_timing.py --build            (no GPU needed) compiles csrc/zkt_poly.hip twice more, once with every product and division forced onto the direct
                                    kernels and once with both forced onto the transform paths, and links each with the objects of the normal build into
                                    zk-toolkit_amd/libzkt_hip_poly_direct.so / libzkt_hip_poly_ntt.so.  The shipped library has no such switch.
  poly_timing.py --out FILE.md      (GPU) sweeps
      * na = nb = 2^4 .. 2^12 products, direct against transform;
      * divisions with L = nb = 2^4 .. 2^12 (na = 2 nb - 1), direct against Newton;
      * the shipped library's transform product at 2^13 .. 2^20 terms per operand, with the achieved GB/s of the byte model
        32 B x N x 2 per k_ntt_group launch x launches per transform x three transforms;
      * the shipped library's zkt_qap_quotient at n = 2^10 .. 2^16, rows = 8.
Both paths are warmed, then alternated for --reps repeats; a host clock runs around blocking calls.  Each row reports median / min / max in ms.
Rule: a threshold is the largest power of two at which the direct path's median is still below the other path's by more than the two paths' own
min-max spread (the larger of the two).  The tables and the outcome are appended to FILE.md."""
import argparse, ctypes, os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "zk-toolkit_amd")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
VARIANTS = {"direct": ("-DZKT_POLY_TIMING_DIRECT=2097152", "-DZKT_POLY_TIMING_DIV=2097152"), "ntt": ("-DZKT_POLY_TIMING_DIRECT=0", "-DZKT_POLY_TIMING_DIV=0")}
lib_path = lambda v: os.path.join(PKG, f"libzkt_hip_poly_{v}.so")

ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true"); ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
ap.add_argument("--max-log", type=int, default=12)
a = ap.parse_args()

if a.build:
    obj = os.path.join(ROOT, "build", "obj"); mine = os.path.join(ROOT, "build", "obj_poly_timing"); os.makedirs(mine, exist_ok=True)
    others = sorted(os.path.join(obj, f) for f in os.listdir(obj) if f.endswith(".o") and f != "zkt_poly.o")
    assert others, "run the normal build first: this links its objects"
    for v, flags in VARIANTS.items():
        o = os.path.join(mine, f"zkt_poly_{v}.o")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result", *flags,
                               "-c", os.path.join(PKG, "csrc", "zkt_poly.hip"), "-o", o])
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_path(v), *others, o, "-ldl"])
        print("built", lib_path(v))
    sys.exit(0)

import torch  # noqa: F401  (one HIP runtime per process, as zk-toolkit_amd/__init__.py explains)
import poly_model as P
assert torch.cuda.is_available(), "the sweep needs the GPU"


def load(path):
    L = ctypes.CDLL(path)
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    L.zkt_fr_poly_mul.argtypes = [vp, sz, vp, sz, vp]; L.zkt_fr_poly_divrem.argtypes = [vp, sz, vp, sz, vp, vp, vp]
    L.zkt_qap_quotient.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    assert L.zkt_init(0) == 0
    return L


LIBS = {v: load(lib_path(v)) for v in VARIANTS}
SHIPPED = load(os.path.join(PKG, "libzkt_hip.so"))
rng = np.random.Generator(np.random.PCG64(5))


def rand(n):
    x = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64); x[:, 3] >>= np.uint64(2); x[-1, 0] |= np.uint64(1)
    return x


p_ = lambda x: x.ctypes.data


def mul_call(L, x, y, out): return lambda: L.zkt_fr_poly_mul(p_(x), len(x), p_(y), len(y), p_(out))


def div_call(L, x, y, q, rem):
    rl = ctypes.c_size_t(0)
    return lambda: L.zkt_fr_poly_divrem(p_(x), len(x), p_(y), len(y), p_(q), p_(rem), ctypes.byref(rl))


def timed(calls, reps):
    """calls: {name: thunk}.  Warm every one, then alternate them; ms per call"""
    for f in calls.values():
        for _ in range(3): assert f() == 0
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter(); rc = f(); t[k].append((time.perf_counter() - t0) * 1e3); assert rc == 0
    return t


fmt = lambda v: "%.3f | %.3f | %.3f" % (statistics.median(v), min(v), max(v))
lines = []


def emit(s):
    print(s, flush=True); lines.append(s)


def sweep(title, make_calls, check):
    emit(f"\n### {title}\n\n| 2^k | direct median | min | max | transform median | min | max | direct wins by more than the spread | same result |\n|---|---|---|---|---|---|---|---|---|")
    best = None
    for k in range(4, a.max_log + 1):
        calls, outs = make_calls(1 << k)
        t = timed(calls, a.reps)
        spread = max(max(t["direct"]) - min(t["direct"]), max(t["ntt"]) - min(t["ntt"]))
        wins = statistics.median(t["ntt"]) - statistics.median(t["direct"]) > spread
        same = check(outs)
        if wins: best = 1 << k
        emit("| %d | %s | %s | %s | %s |" % (k, fmt(t["direct"]), fmt(t["ntt"]), "yes" if wins else "no", "yes" if same else "NO"))
    emit(f"\nRule's outcome: {best if best else 'no size (the direct path never wins by more than the spread)'}")
    return best


def mul_calls(n):
    x, y = rand(n), rand(n); outs = {v: np.zeros((2 * n - 1, 4), np.uint64) for v in VARIANTS}
    return {v: mul_call(LIBS[v], x, y, outs[v]) for v in VARIANTS}, outs


def div_calls(n):
    x, y = rand(2 * n - 1), rand(n); outs = {v: (np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64)) for v in VARIANTS}
    return {v: div_call(LIBS[v], x, y, *outs[v]) for v in VARIANTS}, outs


emit(f"\n## poly_timing.py, {a.reps} repeats per path, alternated, host clock around blocking calls (ms)")
d_mul = sweep("Product, na = nb = 2^k", mul_calls, lambda o: bool((o["direct"] == o["ntt"]).all()))
d_div = sweep("Division, L = nb = 2^k", div_calls, lambda o: all(bool((x == y).all()) for x, y in zip(o["direct"], o["ntt"])))

emit("\n### Transform product of the shipped library, na = nb = 2^k\n\n| 2^k | median | min | max | launches per transform | model bytes | GB/s at the median |\n|---|---|---|---|---|---|---|")
for k in range(13, 21):
    n = 1 << k; x, y = rand(n), rand(n); out = np.zeros((2 * n - 1, 4), np.uint64)
    t = timed({"s": mul_call(SHIPPED, x, y, out)}, a.reps)["s"]
    logN = k + 1; launches = P.ntt_launches(logN); model = 32 * (1 << logN) * 2 * launches * 3
    emit("| %d | %s | %d | %d | %.1f |" % (k, fmt(t), launches, model, model / (statistics.median(t) * 1e-3) / 1e9))

emit("\n### zkt_qap_quotient of the shipped library, rows = 8\n\n| n = 2^k | median | min | max |\n|---|---|---|---|")
for k in range(10, 17):
    n = 1 << k; u, v, w = rand(8 * n), rand(8 * n), rand(8 * n); wires = rand(8); h = np.zeros((n, 4), np.uint64)
    f = lambda: SHIPPED.zkt_qap_quotient(p_(u), p_(v), p_(w), 8, n, p_(wires), p_(h))
    ts = []
    for i in range(3 + a.reps):                       # random inputs leave a remainder: status 5 is the expected end of the same work
        t0 = time.perf_counter(); rc = f(); dt = (time.perf_counter() - t0) * 1e3; assert rc in (0, 5)
        if i >= 3: ts.append(dt)
    emit("| %d | %s |" % (k, fmt(ts)))

src = P.library_constants()
emit(f"\nThe source holds POLY_DIRECT_MAX = {src['POLY_DIRECT_MAX']}, POLY_DIV_DIRECT_MAX = {src['POLY_DIV_DIRECT_MAX']}; the rule gives {d_mul} and {d_div}.")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f: f.write("\n".join(lines) + "\n")
