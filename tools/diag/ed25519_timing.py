#!/usr/bin/env python3
"""Rates of the batched Ed25519 and SHA-512 entry points (csrc/zkt_ed25519.hip), and which build of the verification kernel wins.

  ed25519_timing.py --build           (no GPU needed) builds zk-toolkit_amd/libzkt_hip_ed25519_<variant>.so for every variant below THROUGH THE MAKEFILE
                                      (`make OBJ=../build/obj_ed25519_<variant> LIB=... ED25519FLAGS=...`: the compile and link lines are the Makefile's own; the other
                                      objects of the normal build are copied into the variant's directory, so only zkt_ed25519.o is compiled).
  ed25519_timing.py --out FILE.md     (GPU) measures, at n = 2^10, 2^14, 2^18 over 64-byte messages: zkt_ed25519_verify_batch (host pointers) and
                                      zkt_ed25519_verify_batch_dev (device pointers, the caller's stream, synchronised for the clock), zkt_ed25519_sign_batch,
                                      zkt_ed25519_public_keys_batch, zkt_sha512_batch, and as a yardstick zkt_ecdsa_verify_batch / zkt_ecdsa_verify_digest_batch_dev
                                      at the same n; then the _dev call of every variant that --build made.
Every path is warmed, then the paths are alternated for --reps repeats; a host clock runs around blocking calls.  Each row reports median / min / max in ms.
The signatures are made by zkt_ed25519_sign_batch and are all valid (an invalid one can leave the kernel early); every path's decisions are checked.
The tables are appended to FILE.md."""
import argparse, ctypes, hashlib, os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "zk-toolkit_amd")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
# ED25519FLAGS of each variant (the Makefile's default is waves2)
VARIANTS = {"plain": "", "waves2": "-DZKT_ED25519_WAVES=2", "waves3": "-DZKT_ED25519_WAVES=3", "waves4": "-DZKT_ED25519_WAVES=4",
            "mont": "-DZKT_FE25519_MONT", "mont_waves2": "-DZKT_FE25519_MONT -DZKT_ED25519_WAVES=2", "mont_waves3": "-DZKT_FE25519_MONT -DZKT_ED25519_WAVES=3",
            "lds": "-DZKT_ED25519_TABLE_LDS", "w3_lds": "-DZKT_ED25519_WIN=3 -DZKT_ED25519_TABLE_LDS", "w3": "-DZKT_ED25519_WIN=3", "w5": "-DZKT_ED25519_WIN=5"}
lib_path = lambda v: os.path.join(PKG, f"libzkt_hip_ed25519_{v}.so")

ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--out", default=None)
ap.add_argument("--logs", default="10,14,18"); ap.add_argument("--variants", default=",".join(VARIANTS))
a = ap.parse_args()
chosen = [v for v in a.variants.split(",") if v]

if a.build:
    import shutil
    obj = os.path.join(ROOT, "build", "obj")
    others = sorted(f for f in os.listdir(obj) if f.endswith(".o") and f != "zkt_ed25519.o")
    assert others, "run the normal build first: its objects are reused"
    def build_one(v):
        mine = os.path.join(ROOT, "build", f"obj_ed25519_{v}"); os.makedirs(mine, exist_ok=True)
        for f in others: shutil.copy2(os.path.join(obj, f), os.path.join(mine, f))          # timestamps kept: make finds them up to date
        subprocess.check_call(["make", "-s", "-C", PKG, f"OBJ=../build/obj_ed25519_{v}", f"LIB={os.path.basename(lib_path(v))}", f"ED25519FLAGS={VARIANTS[v]}", os.path.basename(lib_path(v))])
        return lib_path(v)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=5) as ex:
        for built in ex.map(build_one, chosen): print("built", built)
    sys.exit(0)

import torch
assert torch.cuda.is_available(), "the sweep needs the GPU"
zk = __import__("importlib").import_module("zk-toolkit_amd")
zk.init(0)
L = zk.lib()
p_ = lambda x: x.ctypes.data
fmt = lambda v: "%.3f | %.3f | %.3f" % (statistics.median(v), min(v), max(v))
med = statistics.median
lines = []


def emit(s):
    print(s, flush=True); lines.append(s)


def timed(calls, reps):
    """calls: {name: thunk}.  Warm every one, then alternate them; ms per call"""
    for f in calls.values():
        for _ in range(2): f()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); t[k].append((time.perf_counter() - t0) * 1e3)
    return t


def workload(n, msg_len=64, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    buf = rng.integers(0, 256, size=n * msg_len, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(msg_len)
    prv = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    pub = np.zeros((n, 32), np.uint8); sig = np.zeros((n, 64), np.uint8)
    assert L.zkt_ed25519_public_keys_batch(p_(prv), n, p_(pub)) == 0 and L.zkt_ed25519_sign_batch(p_(buf), p_(off), p_(prv), n, p_(sig)) == 0
    return buf, off, prv, pub, sig


def dev_call(lib, buf, off, sig, pub, n):
    d = [torch.from_numpy(x).cuda() for x in (buf, off.view(np.int64), sig, pub)]
    d_ok = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    def f():
        rc = lib.zkt_ed25519_verify_batch_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_ok.data_ptr(), s)
        torch.cuda.synchronize()
        return rc
    return f, d_ok, d


def ecdsa_workload(n, buf, off):
    rng = np.random.Generator(np.random.PCG64(2))
    sks = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64); ks = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64)
    sigs = np.zeros((n, 8), np.uint64); retry = np.zeros(n, np.uint32); pks = np.zeros((n, 9), np.uint64)
    assert L.zkt_ecdsa_sign_batch(p_(buf), p_(off), p_(sks), p_(ks), n, p_(sigs), p_(retry)) == 0 and not retry.any()
    assert L.zkt_ecdsa_public_keys_batch(p_(sks), n, p_(pks)) == 0
    return sigs, pks


emit(f"\n## ed25519_timing.py, {a.reps} repeats per path, alternated, host clock around blocking calls (ms)")
emit("\n### n elements over 64-byte messages (the shipped library); median | min | max\n\n| n = 2^k | verify_batch | | | verify_batch_dev | | | sign_batch | | | public_keys_batch | | | sha512_batch | | | "
     "ecdsa_verify_batch | | | ecdsa_verify_digest_batch_dev | | | verifications/s (host) | verifications/s (_dev) | signatures/s | keys/s | SHA-512 MB/s | ECDSA verifications/s (_dev) | checked |\n" + "|---" * 29 + "|")
for k in [int(x) for x in a.logs.split(",")]:
    n = 1 << k
    buf, off, prv, pub, sig = workload(n)
    ok_host = np.zeros(n, np.uint32); pub2 = np.zeros_like(pub); sig2 = np.zeros_like(sig); dig = np.zeros((n, 64), np.uint8); ok_e = np.zeros(n, np.uint32)
    esig, epk = ecdsa_workload(n, buf, off)
    edig = np.frombuffer(b"".join(hashlib.sha256(buf[i * 64:(i + 1) * 64].tobytes()).digest() for i in range(n)), dtype=np.uint8).copy()
    d_e = [torch.from_numpy(x).cuda() for x in (edig, esig.view(np.int64), epk.view(np.int64))]; d_eok = torch.zeros(n, dtype=torch.int32, device="cuda")
    s0 = torch.cuda.current_stream().cuda_stream
    fdev, d_ok, _keep = dev_call(L, buf, off, sig, pub, n)
    def f_dev(): assert fdev() == 0
    def f_host(): assert L.zkt_ed25519_verify_batch(p_(buf), p_(off), p_(sig), p_(pub), n, p_(ok_host)) == 0
    def f_sign(): assert L.zkt_ed25519_sign_batch(p_(buf), p_(off), p_(prv), n, p_(sig2)) == 0
    def f_pub(): assert L.zkt_ed25519_public_keys_batch(p_(prv), n, p_(pub2)) == 0
    def f_sha(): assert L.zkt_sha512_batch(p_(buf), p_(off), n, p_(dig)) == 0
    def f_ecdsa(): assert L.zkt_ecdsa_verify_batch(p_(buf), p_(off), p_(esig), p_(epk), n, p_(ok_e)) == 0
    def f_ecdsa_dev():
        assert L.zkt_ecdsa_verify_digest_batch_dev(d_e[0].data_ptr(), d_e[1].data_ptr(), d_e[2].data_ptr(), n, d_eok.data_ptr(), s0) == 0
        torch.cuda.synchronize()
    t = timed({"host": f_host, "dev": f_dev, "sign": f_sign, "pub": f_pub, "sha": f_sha, "ecdsa": f_ecdsa, "ecdsa_dev": f_ecdsa_dev}, a.reps)
    good = bool(ok_host.all()) and bool(d_ok.cpu().numpy().all()) and (sig2 == sig).all() and (pub2 == pub).all() and bool(ok_e.all()) and bool(d_eok.cpu().numpy().all()) and \
        all(dig[i].tobytes() == hashlib.sha512(buf[i * 64:(i + 1) * 64].tobytes()).digest() for i in range(min(n, 256)))
    m = {x: med(t[x]) for x in t}
    emit("| %d | %s | %s | %s | %s | %s | %s | %s | %.0f | %.0f | %.0f | %.0f | %.1f | %.0f | %s |" % (
        k, fmt(t["host"]), fmt(t["dev"]), fmt(t["sign"]), fmt(t["pub"]), fmt(t["sha"]), fmt(t["ecdsa"]), fmt(t["ecdsa_dev"]),
        n / m["host"] * 1e3, n / m["dev"] * 1e3, n / m["sign"] * 1e3, n / m["pub"] * 1e3, n * 64 / m["sha"] * 1e3 / 1e6, n / m["ecdsa_dev"] * 1e3, "yes" if good else "NO"))

have = [v for v in chosen if os.path.exists(lib_path(v))]
libs = {}
for v in have:
    lib = ctypes.CDLL(lib_path(v)); lib.zkt_ed25519_verify_batch_dev.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    assert lib.zkt_init(0) == 0
    libs[v] = lib
for k in ((14, 18) if have else ()):
    n = 1 << k
    buf, off, prv, pub, sig = workload(n)
    calls, oks, refused, keep = {}, {}, {}, []
    for v in have:
        f, oks[v], d = dev_call(libs[v], buf, off, sig, pub, n); keep.append(d)
        rc = f()                                    # a build whose block the runtime does not launch reports a status here and is left out of the timing
        if rc == 0: calls[v] = f
        else: refused[v] = rc
    t = timed(calls, a.reps)
    emit("\n### Builds of k_ed25519_verify, zkt_ed25519_verify_batch_dev at n = 2^%d\n\n| variant | ED25519FLAGS | median | min | max | verifications/s | all accepted |\n|---|---|---|---|---|---|---|" % k)
    for v in have:
        if v in refused: emit("| %s | %s | did not launch (status %d) | | | | |" % (v, VARIANTS[v] or "(empty)", refused[v])); continue
        emit("| %s | %s | %s | %.0f | %s |" % (v, VARIANTS[v] or "(empty)", fmt(t[v]), n / med(t[v]) * 1e3, "yes" if oks[v].cpu().numpy().all() else "NO"))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f: f.write("\n".join(lines) + "\n")
