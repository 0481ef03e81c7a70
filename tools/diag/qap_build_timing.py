#!/usr/bin/env python3
"""What the R1CS -> QAP build on the device (csrc/zkt_qap.hip) costs, and what a resident QAP saves on the way to a proof.

  qap_build_timing.py --out FILE.md      (GPU)
      (a) zkt_qap_create on chain_circuit_sparse and asym_circuit_sparse at n = 256, 1024, 4096 and the largest n whose cols * n fits ZKT_QAP_MAX_CELLS
          (cols = n + 2 and n + 6, so n = 8191 and 8189: n = 8192 itself exceeds the cell limit with either circuit), with the device time of k_qap_basis
          and k_qap_columns from zkt_qap_last_build_ms (events around the two launches);
      (b) the achieved bandwidth of k_qap_columns against the byte model 32 B x (nnz * n + 3 * cols * n), nnz over the three matrices;
      (c) R1CS -> CRS -> proof at n = 1024 and 4096: zkt_qap_create + zkt_groth16_setup_resident + zkt_groth16_prove_resident against zkt_groth16_setup +
          zkt_groth16_prove_qap fed the same three arrays from host memory (the interface before the resident handle; its arrays are taken as given, so
          the comparison leaves out whatever built them on the host).
Every path is warmed, then the paths of a table are alternated for --reps repeats; a host clock runs around blocking calls.  Rows report median / min / max in
ms.  The tables are appended to FILE.md."""
import argparse, ctypes, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
ap.add_argument("--sizes", default="256,1024,4096,max"); ap.add_argument("--proof-sizes", default="1024,4096")
a = ap.parse_args()

import importlib
import torch  # noqa: F401  (one HIP runtime per process, as zk-toolkit_amd/__init__.py explains)
from qap_util import chain_circuit_sparse, asym_circuit_sparse, sparse_struct, alloc_crs
from zkt_testlib import ints_to_arr, SplitMix64, R
assert torch.cuda.is_available(), "the sweep needs the GPU"
zk = importlib.import_module("zk-toolkit_amd")
zk.init(0)
L = zk.lib()
MAX_CELLS = 1 << 26
HBM_COPY_TBS = 6.29            # measured copy rate of the MI355X micro-architecture notes, TB/s

CIRCUITS = {"chain": (chain_circuit_sparse, 2), "asym": (asym_circuit_sparse, 6)}      # cols = n + extra
fmt = lambda v: "%.3f | %.3f | %.3f" % (statistics.median(v), min(v), max(v))
lines = []


def emit(s):
    print(s, flush=True); lines.append(s)


def largest_n(extra):
    n = 8192
    while n * (n + extra) > MAX_CELLS: n -= 1
    return n


def instance(name, n):
    make, extra = CIRCUITS[name]
    mats, wires, l, m = make(n)
    assert m + 1 == n + extra
    return {"n": n, "cols": m + 1, "l": l, "m": m, "wires": wires, "structs": [sparse_struct(*M) for M in mats], "nnz": sum(int(M[0][n]) for M in mats)}


def create(c):
    h = ctypes.c_void_p()
    rc = L.zkt_qap_create(c["n"], c["cols"], *[ctypes.byref(s) for s in c["structs"]], ctypes.byref(h))
    assert rc == 0, rc
    return h


def timed(calls, reps):
    """calls: {name: thunk returning extra figures or None}.  Warm every one, then alternate them; ms per call and the figures of every repeat"""
    for f in calls.values():
        for _ in range(2): f()
    t = {k: [] for k in calls}; extra = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter(); x = f(); t[k].append((time.perf_counter() - t0) * 1e3); extra[k].append(x)
    return t, extra


def build_call(c):
    def f():
        h = create(c)
        b, k = ctypes.c_float(), ctypes.c_float()
        L.zkt_qap_last_build_ms(ctypes.byref(b), ctypes.byref(k))
        L.zkt_qap_free(h)
        return b.value, k.value
    return f


emit(f"\n## qap_build_timing.py, {a.reps} repeats per path, alternated, host clock around blocking calls (ms)")
emit("\n### (a), (b) zkt_qap_create (+ zkt_qap_free): whole call on the host clock; k_qap_basis and k_qap_columns on device events\n")
emit("| circuit | n | cols | nnz | call median | min | max | k_qap_basis median | k_qap_columns median | basis share of the two | model bytes of k_qap_columns | GB/s at the median | of the 6.29 TB/s copy rate |")
emit("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
shares = {}
for tok in a.sizes.split(","):
    cs = {name: instance(name, largest_n(extra) if tok == "max" else int(tok)) for name, (_, extra) in CIRCUITS.items()}
    t, ex = timed({name: build_call(c) for name, c in cs.items()}, a.reps)
    for name, c in cs.items():
        basis = statistics.median(x[0] for x in ex[name]); colms = statistics.median(x[1] for x in ex[name])
        model = 32 * (c["nnz"] * c["n"] + 3 * c["cols"] * c["n"])
        gbs = model / (colms * 1e-3) / 1e9
        shares[(name, c["n"])] = basis / (basis + colms)
        emit("| %s | %d | %d | %d | %s | %.3f | %.3f | %.0f %% | %d | %.1f | %.1f %% |" % (name, c["n"], c["cols"], c["nnz"], fmt(t[name]), basis, colms, 100 * basis / (basis + colms), model, gbs,
                                                                                  100 * gbs / (HBM_COPY_TBS * 1e3)))

emit("\n### (c) R1CS -> CRS -> proof in coefficient form\n")
emit("resident: zkt_qap_create, zkt_groth16_setup_resident, zkt_groth16_prove_resident, zkt_qap_free.  host arrays: zkt_groth16_setup, zkt_groth16_prove_qap on ui, vi, wi in host memory.\n")
emit("| circuit | n | bytes of ui + vi + wi | resident median | min | max | host arrays median | min | max | same proof |")
emit("|---|---|---|---|---|---|---|---|---|---|")
p_ = lambda x: x.ctypes.data
for tok in a.proof_sizes.split(","):
    n = int(tok)
    for name in CIRCUITS:
        c = instance(name, n); cols, l, m = c["cols"], c["l"], c["m"]
        rng = SplitMix64(n + len(name))
        trap = [ints_to_arr([rng.below(R - 1) + 1], 4) for _ in range(4)] + [ints_to_arr([rng.below(R - 3 * n) + 2 * n], 4)]
        r, s = ints_to_arr([rng.below(R - 1) + 1], 4), ints_to_arr([rng.below(R - 1) + 1], 4)
        h = create(c)
        uvw = [np.zeros((cols * n, 4), np.uint64) for _ in range(3)]
        assert L.zkt_qap_download(h, *[p_(x) for x in uvw]) == 0
        L.zkt_qap_free(h)
        proofs = {k: [np.zeros((1, 13), np.uint64), np.zeros((1, 25), np.uint64), np.zeros((1, 13), np.uint64)] for k in ("resident", "host")}
        crs = {k: alloc_crs(n, l, m) for k in proofs}
        def resident():
            q = create(c)
            assert L.zkt_groth16_setup_resident(ctypes.byref(crs["resident"][0]), q, *[p_(t) for t in trap]) == 0
            assert L.zkt_groth16_prove_resident(ctypes.byref(crs["resident"][0]), q, p_(c["wires"]), p_(r), p_(s), *[p_(x) for x in proofs["resident"]]) == 0
            L.zkt_qap_free(q)
        def host():
            assert L.zkt_groth16_setup(ctypes.byref(crs["host"][0]), *[p_(x) for x in uvw], *[p_(t) for t in trap]) == 0
            assert L.zkt_groth16_prove_qap(ctypes.byref(crs["host"][0]), *[p_(x) for x in uvw], p_(c["wires"]), p_(r), p_(s), *[p_(x) for x in proofs["host"]]) == 0
        t, _ = timed({"resident": resident, "host": host}, a.reps)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(proofs["resident"], proofs["host"]))
        emit("| %s | %d | %d | %s | %s | %s |" % (name, n, 3 * cols * n * 32, fmt(t["resident"]), fmt(t["host"]), "yes" if same else "NO"))

at4096 = {k: v for k, v in shares.items() if k[1] == 4096}
if at4096:
    emit("\nBasis share of the two kernels at n = 4096: " + ", ".join("%s %.0f %%" % (k[0], 100 * v) for k, v in at4096.items()) +
         ".  The division is chunked (csrc/zkt_qap.hip) only where this share is the larger one.")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f: f.write("\n".join(lines) + "\n")
