#!/usr/bin/env python3
"""What the fused ECDSA verification (csrc/zkt_ecdsa.hip) buys over the composition of the public calls it replaces, and which build of its kernel wins.

  ecdsa_timing.py --build           (no GPU needed) builds zk-toolkit_amd/libzkt_hip_ecdsa_<variant>.so for every variant below THROUGH THE MAKEFILE
                                    (`make OBJ=../build/obj_ecdsa_<variant> LIB=... ECDSAFLAGS=...`: the compile and link lines are the Makefile's own; the other
                                    objects of the normal build are copied into the variant's directory, so only zkt_ecdsa.o is compiled).  The shipped library has
                                    no such switch.
  ecdsa_timing.py --out FILE.md     (GPU) measures, at n = 2^10, 2^14, 2^16, 2^18 signatures over 64-byte messages,
      * zkt_ecdsa_verify_batch (host pointers, hashes on the device),
      * zkt_ecdsa_verify_digest_batch_dev (device pointers, the caller's stream, synchronised for the clock),
      * the composition: hashlib on the host, zkt_sn_inv_batch, two zkt_sn_mul_batch, two zkt_secp_mul_batch (the generator repeated n times),
        zkt_secp_add_batch and a vectorised host compare x == r (the exact x mod n == r on python integers runs once, outside the clock); the host hash
        loop is also timed alone, so that the table shows how much of the composition it is;
    then the _dev call of every variant that --build made, at n = 2^16 and 2^18; then zkt_sha256_batch at 64-byte and 1 KiB messages with its byte rate.
Every path is warmed, then the paths are alternated for --reps repeats; a host clock runs around blocking calls.  Each row reports median / min / max in ms.
The signatures are made by zkt_ecdsa_sign_batch and are all valid (an invalid r or s leaves the kernel early; a valid one runs it to the end); every path's decisions are
compared.  The tables are appended to FILE.md."""
import argparse, ctypes, hashlib, os, statistics, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "zk-toolkit_amd")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
# ECDSAFLAGS of each variant (the Makefile's default is w4_inline).  *_lds: the table of Q in LDS, 64 lanes interleaved (92,160 B per block at 4 bits, 43,008 B at 3)
VARIANTS = {"w3": "-DZKT_ECDSA_WIN=3", "w4": "", "w5": "-DZKT_ECDSA_WIN=5",
            "w3_inline": "-DZKT_INLINE_MUL -DZKT_ECDSA_WIN=3", "w4_inline": "-DZKT_INLINE_MUL", "w5_inline": "-DZKT_INLINE_MUL -DZKT_ECDSA_WIN=5",
            "w3_inline_lds": "-DZKT_INLINE_MUL -DZKT_ECDSA_WIN=3 -DZKT_ECDSA_TABLE_LDS", "w4_inline_lds": "-DZKT_INLINE_MUL -DZKT_ECDSA_TABLE_LDS"}
lib_path = lambda v: os.path.join(PKG, f"libzkt_hip_ecdsa_{v}.so")

ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--out", default=None)
ap.add_argument("--logs", default="10,14,16,18")
a = ap.parse_args()

if a.build:
    import shutil
    obj = os.path.join(ROOT, "build", "obj")
    others = sorted(f for f in os.listdir(obj) if f.endswith(".o") and f != "zkt_ecdsa.o")
    assert others, "run the normal build first: its objects are reused"
    def build_one(v):
        mine = os.path.join(ROOT, "build", f"obj_ecdsa_{v}"); os.makedirs(mine, exist_ok=True)
        for f in others: shutil.copy2(os.path.join(obj, f), os.path.join(mine, f))          # timestamps kept: make finds them up to date
        subprocess.check_call(["make", "-s", "-C", PKG, f"OBJ=../build/obj_ecdsa_{v}", f"LIB={os.path.basename(lib_path(v))}", f"ECDSAFLAGS={VARIANTS[v]}", os.path.basename(lib_path(v))])
        return lib_path(v)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as ex:
        for built in ex.map(build_one, VARIANTS): print("built", built)
    sys.exit(0)

import torch
from zkt_testlib import SECP_GEN, SECP_N, secp_arr, limbs_to_int
assert torch.cuda.is_available(), "the sweep needs the GPU"
zk = __import__("importlib").import_module("zk-toolkit_amd")
zk.init(0)
L = zk.lib()
p_ = lambda x: x.ctypes.data
# the existing calls of the composition have no argument types in the loader: declared here, or a 64-bit address handed over as a python int travels as a C int
vp_, sz_ = ctypes.c_void_p, ctypes.c_size_t
L.zkt_sn_inv_batch.argtypes = [vp_, vp_, sz_]; L.zkt_sn_mul_batch.argtypes = [vp_, vp_, vp_, sz_]
L.zkt_secp_mul_batch.argtypes = [vp_, vp_, ctypes.c_int, vp_, sz_]; L.zkt_secp_add_batch.argtypes = [vp_, vp_, vp_, sz_]
fmt = lambda v: "%.3f | %.3f | %.3f" % (statistics.median(v), min(v), max(v))
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
    off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(msg_len))
    sks = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64); ks = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64)
    sigs = np.zeros((n, 8), np.uint64); retry = np.zeros(n, np.uint32); pks = np.zeros((n, 9), np.uint64)
    assert L.zkt_ecdsa_sign_batch(p_(buf), p_(off), p_(sks), p_(ks), n, p_(sigs), p_(retry)) == 0 and not retry.any()
    assert L.zkt_ecdsa_public_keys_batch(p_(sks), n, p_(pks)) == 0
    return buf, off, sigs, pks


def host_hash(buf, n, msg_len):
    """z of every message as four little-endian limbs, hashed on the host as a python caller of the parent commit would"""
    raw = buf.tobytes()
    zb = b"".join(hashlib.sha256(raw[i * msg_len:(i + 1) * msg_len]).digest()[::-1] for i in range(n))      # big-endian digest -> little-endian limbs
    return np.frombuffer(zb, dtype=np.uint64).reshape(n, 4).copy()


def composition(buf, off, sigs, pks, n, msg_len):
    """the parent commit's capability: seven round trips and a host hash.  Returns (decisions by the vectorised compare x == r, the sum's points)"""
    z = host_hash(buf, n, msg_len)
    r, s = np.ascontiguousarray(sigs[:, :4]), np.ascontiguousarray(sigs[:, 4:])
    w, u1, u2 = (np.zeros((n, 4), np.uint64) for _ in range(3))
    p1, p2, p3 = (np.zeros((n, 9), np.uint64) for _ in range(3))
    gens = np.repeat(secp_arr([SECP_GEN]), n, axis=0)
    assert L.zkt_sn_inv_batch(p_(s), p_(w), n) == 0 and L.zkt_sn_mul_batch(p_(z), p_(w), p_(u1), n) == 0 and L.zkt_sn_mul_batch(p_(r), p_(w), p_(u2), n) == 0
    assert L.zkt_secp_mul_batch(p_(gens), p_(u1), 4, p_(p1), n) == 0 and L.zkt_secp_mul_batch(p_(pks), p_(u2), 4, p_(p2), n) == 0
    assert L.zkt_secp_add_batch(p_(p1), p_(p2), p_(p3), n) == 0
    return (p3[:, 8] == 0) & (p3[:, :4] == r).all(axis=1), p3      # x == r: misses only x >= n (probability 2^-128 for a valid signature); the exact compare is outside the clock


def composition_exact(p3, sigs, n):
    """x mod n == r on python integers, first 4096 elements: not timed"""
    return all(p3[i, 8] == 0 and limbs_to_int(p3[i, :4]) % SECP_N == limbs_to_int(sigs[i, :4]) for i in range(min(n, 4096)))


def dev_call(lib, dig, sigs, pks, n):
    d_dig, d_sig, d_pk = torch.from_numpy(dig).cuda(), torch.from_numpy(sigs.view(np.int64)).cuda(), torch.from_numpy(pks.view(np.int64)).cuda()
    d_ok = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    def f():
        rc = lib.zkt_ecdsa_verify_digest_batch_dev(d_dig.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), n, d_ok.data_ptr(), s)
        torch.cuda.synchronize()
        return rc
    return f, d_ok


emit(f"\n## ecdsa_timing.py, {a.reps} repeats per path, alternated, host clock around blocking calls (ms)")
emit("\n### Verification of n signatures over 64-byte messages (the shipped library)\n\n| n = 2^k | zkt_ecdsa_verify_batch median | min | max | _digest_batch_dev median | min | max | composition median | min | max | "
     "its host hash loop alone, median | composition / verify_batch | (composition - host hash) / verify_batch | signatures/s (verify_batch) | signatures/s (_dev) | same decisions |\n" + "|---" * 16 + "|")
for k in [int(x) for x in a.logs.split(",")]:
    n = 1 << k
    buf, off, sigs, pks = workload(n)
    dig = np.frombuffer(b"".join(hashlib.sha256(buf[i * 64:(i + 1) * 64].tobytes()).digest() for i in range(n)), dtype=np.uint8).copy()
    ok_host = np.zeros(n, np.uint32); res = {}
    fdev, d_ok = dev_call(L, dig, sigs, pks, n)
    def f_dev(): assert fdev() == 0
    def f_host(): assert L.zkt_ecdsa_verify_batch(p_(buf), p_(off), p_(sigs), p_(pks), n, p_(ok_host)) == 0
    def f_comp(): res["c"] = composition(buf, off, sigs, pks, n, 64)
    def f_hash(): host_hash(buf, n, 64)
    t = timed({"host": f_host, "dev": f_dev, "comp": f_comp, "hash": f_hash}, a.reps if k < 18 else min(a.reps, 3))
    same = bool(ok_host.all()) and bool(d_ok.cpu().numpy().all()) and bool(res["c"][0].all()) and composition_exact(res["c"][1], sigs, n)
    mh, md, mc, mz = (statistics.median(t[x]) for x in ("host", "dev", "comp", "hash"))
    emit("| %d | %s | %s | %s | %.3f | %.2f | %.2f | %.0f | %.0f | %s |" % (k, fmt(t["host"]), fmt(t["dev"]), fmt(t["comp"]), mz, mc / mh, (mc - mz) / mh, n / mh * 1e3, n / md * 1e3, "yes" if same else "NO"))

have = [v for v in VARIANTS if os.path.exists(lib_path(v))]
libs = {}
for v in have:
    lib = ctypes.CDLL(lib_path(v)); lib.zkt_ecdsa_verify_digest_batch_dev.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    assert lib.zkt_init(0) == 0
    libs[v] = lib
for k in ((16, 18) if have else ()):
    n = 1 << k
    buf, off, sigs, pks = workload(n)
    dig = np.frombuffer(b"".join(hashlib.sha256(buf[i * 64:(i + 1) * 64].tobytes()).digest() for i in range(n)), dtype=np.uint8).copy()
    calls, oks, refused = {}, {}, {}
    for v in have:
        f, oks[v] = dev_call(libs[v], dig, sigs, pks, n)
        rc = f()                                    # a build whose block the runtime does not launch reports a status here and is left out of the timing
        if rc == 0: calls[v] = f
        else: refused[v] = rc
    t = timed(calls, a.reps)
    emit("\n### Builds of k_ecdsa_verify, zkt_ecdsa_verify_digest_batch_dev at n = 2^%d\n\n| variant | ECDSAFLAGS | median | min | max | signatures/s | all accepted |\n|---|---|---|---|---|---|---|" % k)
    for v in have:
        if v in refused: emit("| %s | %s | did not launch (status %d) | | | | |" % (v, VARIANTS[v] or "(empty: called multiply)", refused[v])); continue
        emit("| %s | %s | %s | %.0f | %s |" % (v, VARIANTS[v] or "(empty: called multiply)", fmt(t[v]), n / statistics.median(t[v]) * 1e3, "yes" if oks[v].cpu().numpy().all() else "NO"))

emit("\n### zkt_sha256_batch (host pointers: upload, one lane per message, download)\n\n| message bytes | messages | median | min | max | GB/s of message bytes at the median | same as hashlib (first 256) |\n|---|---|---|---|---|---|---|")
for msg_len, n in ((64, 1 << 18), (1024, 1 << 16)):
    rng = np.random.Generator(np.random.PCG64(3))
    buf = rng.integers(0, 256, size=n * msg_len, dtype=np.uint8); off = np.arange(n + 1, dtype=np.uint64) * np.uint64(msg_len); out = np.zeros((n, 32), np.uint8)
    def f_sha(): assert L.zkt_sha256_batch(p_(buf), p_(off), n, p_(out)) == 0
    t = timed({"s": f_sha}, a.reps)["s"]
    same = all(out[i].tobytes() == hashlib.sha256(buf[i * msg_len:(i + 1) * msg_len].tobytes()).digest() for i in range(256))
    emit("| %d | %d | %s | %.2f | %s |" % (msg_len, n, fmt(t), n * msg_len / (statistics.median(t) * 1e-3) / 1e9, "yes" if same else "NO"))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f: f.write("\n".join(lines) + "\n")
