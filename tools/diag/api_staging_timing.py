#!/usr/bin/env python3
"""Host overhead of the staged host-pointer calls (csrc/host_stage.h: Stage), this tree's library against another build of it in ONE process.

  api_staging_timing.py --parent PATH/libzkt_hip_parent.so [--reps 9] [--out FILE.md]     (GPU)

The other library is built from the commit to compare with (`git archive <commit> | tar -x -C DIR && make -C DIR/zk-toolkit_amd`) and loaded beside the tree's own;
each has its own zkt_init, stream and arena.  Per shape both are warmed, then alternated for --reps repeats with a host clock around each blocking call; each
row reports median | min | max in ms per library and whether this tree's median lies inside the other library's own min-max.  Both libraries' results are compared.
The table is appended to FILE.md."""
import argparse, ctypes, hashlib, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.reps >= 7

vp, sz = ctypes.c_void_p, ctypes.c_size_t
SIGS = {"zkt_fr_mul_batch": [vp, vp, vp, sz], "zkt_secp_sum": [vp, sz, vp], "zkt_secp_mul_batch": [vp, vp, ctypes.c_int, vp, sz], "zkt_sha512_batch": [vp, vp, sz, vp],
        "zkt_ed25519_public_keys_batch": [vp, sz, vp], "zkt_ed25519_sign_batch": [vp, vp, vp, sz, vp], "zkt_ed25519_verify_batch": [vp, vp, vp, vp, sz, vp]}


def load(path):
    lib = ctypes.CDLL(path)
    for name, args in SIGS.items(): getattr(lib, name).argtypes = args
    assert lib.zkt_init(0) == 0, "the comparison needs the GPU"
    return lib


LIBS = {"parent": load(a.parent), "branch": load(os.path.join(ROOT, "zk-toolkit_amd", "libzkt_hip.so"))}
B = LIBS["branch"]
p_ = lambda x: x.ctypes.data
fmt = lambda v: "%.3f | %.3f | %.3f" % (statistics.median(v), min(v), max(v))
rng = np.random.Generator(np.random.PCG64(5))
lines = []


def emit(s):
    print(s, flush=True); lines.append(s)


def fr_mul(n):
    x = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64); y = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    x[:, 3] >>= np.uint64(2); y[:, 3] >>= np.uint64(2)                     # canonical: below 2^254
    out = {k: np.zeros((n, 4), np.uint64) for k in LIBS}
    return {k: (lambda k=k: LIBS[k].zkt_fr_mul_batch(p_(x), p_(y), p_(out[k]), n)) for k in LIBS}, out


def secp_sum(n):
    from zkt_testlib import secp_arr, SECP_GEN
    g = np.repeat(secp_arr([SECP_GEN]), n, axis=0); k = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64); pts = np.zeros((n, 9), np.uint64)
    assert B.zkt_secp_mul_batch(p_(g), p_(k), 4, p_(pts), n) == 0
    out = {k: np.zeros((1, 9), np.uint64) for k in LIBS}
    return {k: (lambda k=k: LIBS[k].zkt_secp_sum(p_(pts), n, p_(out[k]))) for k in LIBS}, out


def messages(n):
    return rng.integers(0, 256, size=n * 64, dtype=np.uint8), np.arange(n + 1, dtype=np.uint64) * np.uint64(64)


def sha512(n):
    buf, off = messages(n)
    out = {k: np.zeros((n, 64), np.uint8) for k in LIBS}
    calls = {k: (lambda k=k: LIBS[k].zkt_sha512_batch(p_(buf), p_(off), n, p_(out[k]))) for k in LIBS}
    return calls, out, lambda o: all(o[i].tobytes() == hashlib.sha512(buf[64 * i:64 * i + 64].tobytes()).digest() for i in range(0, n, 257))


def ed_verify(n):
    buf, off = messages(n)
    prv = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); pub = np.zeros((n, 32), np.uint8); sig = np.zeros((n, 64), np.uint8)
    assert B.zkt_ed25519_public_keys_batch(p_(prv), n, p_(pub)) == 0 and B.zkt_ed25519_sign_batch(p_(buf), p_(off), p_(prv), n, p_(sig)) == 0
    out = {k: np.zeros(n, np.uint32) for k in LIBS}
    calls = {k: (lambda k=k: LIBS[k].zkt_ed25519_verify_batch(p_(buf), p_(off), p_(sig), p_(pub), n, p_(out[k]))) for k in LIBS}
    return calls, out, lambda o: bool(o.all())


emit(f"\n## api_staging_timing.py, {a.reps} repeats per library, alternated, host clock around each blocking call (ms); median | min | max")
emit("\n| call | parent | | | branch | | | branch median inside the parent's min-max | results equal and checked |\n" + "|---" * 9 + "|")
for label, made in [("zkt_fr_mul_batch n = 1", fr_mul(1)), ("zkt_fr_mul_batch n = 2^20", fr_mul(1 << 20)), ("zkt_secp_sum n = 2^12", secp_sum(1 << 12)),
                    ("zkt_sha512_batch 2^16 x 64 B", sha512(1 << 16)), ("zkt_ed25519_verify_batch n = 2^14", ed_verify(1 << 14))]:
    calls, out, check = made if len(made) == 3 else (*made, lambda o: True)
    for f in calls.values():
        for _ in range(2): assert f() == 0
    t = {k: [] for k in calls}
    for r in range(a.reps):
        for k, f in list(calls.items())[::-1 if r % 2 else 1]:             # who goes first changes every repeat: the second caller finds the inputs in the host's caches
            t0 = time.perf_counter(); rc = f(); t[k].append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
    m = statistics.median(t["branch"])
    good = (out["parent"] == out["branch"]).all() and check(out["branch"])
    emit("| %s | %s | %s | %s | %s |" % (label, fmt(t["parent"]), fmt(t["branch"]), "yes" if min(t["parent"]) <= m <= max(t["parent"]) else "NO: %s" % ("below its min (faster)" if m < min(t["parent"]) else "above its max (slower)"), "yes" if good else "NO"))
for lib in LIBS.values(): lib.zkt_shutdown()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f: f.write("\n".join(lines) + "\n")
