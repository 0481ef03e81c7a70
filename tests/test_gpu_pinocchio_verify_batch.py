"""zkt_pinocchio_verify_batch (a resident verification key, n proofs per call; csrc/zkt_pinocchio_verify.hip) against
  - tests/pinocchio_verify_model.py (Verifier::verify on discrete logarithms, pinned to the oracle by tests/test_pinocchio_verify_model.py) on keys and proofs built
    from known exponents, at batch sizes around the wave size, and
  - zkt_pinocchio_verify, the one-proof call that tests/test_gpu_pinocchio.py pins to the oracle, on real instances and on points outside their groups.
The last test runs the whole module once more in a child process with the small-batch kernels switched off, so that every n takes the one-proof-per-lane kernels."""
import ctypes, importlib, os, subprocess, sys
import numpy as np
import pytest
from zkt_testlib import *
from qap_util import *
import pinocchio_verify_model as M

pytestmark = pytest.mark.gpu
zk = importlib.import_module("zk-toolkit_amd")
O = oracle()
G2_FIELDS = ("g2_w_mid_s", "h_s")
KEY_FIELDS = (("one2", "one_g2", 1), ("alpha_v", "alpha_v", 1), ("alpha_w", "alpha_w", 0), ("alpha_y", "alpha_y", 1), ("gamma", "gamma", 1), ("beta_gamma", "beta_gamma", 1),
              ("t", "t", 0))


@pytest.fixture(scope="module")
def L():
    zk.init()
    return zk.lib()


def points(L, exps, g2):
    """generator * e for every e (G1 through the comb table, G2 through the batched multiplication); exponent 0 is the point at infinity"""
    n = len(exps)
    k = ints_to_arr([e % R or 1 for e in exps], 4)
    if g2:
        gen = np.zeros((1, G2W), np.uint64); O.zkto_g2_generator(ptr(gen))
        out = np.zeros((n, G2W), np.uint64)
        zk.check(L.zkt_g2_mul_batch(ptr(np.repeat(gen, n, axis=0)), ptr(k), 4, ptr(out), n))
    else:
        out = np.zeros((n, G1W), np.uint64)
        zk.check(L.zkt_bls_public_keys_batch(ptr(k), n, ptr(out)))
    for i, e in enumerate(exps):
        if e % R == 0: out[i] = 0; out[i, -1] = 1
    return out


def key_struct(L, key):
    """a zkt_pinocchio_crs whose VerificationKeys fields are generator * the model key's exponents (nothing else is read by either verifier)"""
    crs, buf = alloc_pinocchio(4, len(key["vk"]), 1, 1)
    for name, field, g2 in KEY_FIELDS: buf[field][:] = points(L, [key[name]], g2)
    if key["vk"]:
        buf["vk_io"][:] = points(L, key["vk"], 0); buf["wk_io"][:] = points(L, key["wk"], 1); buf["yk_io"][:] = points(L, key["yk"], 0)
    return crs, buf


class Handle:
    def __init__(self, L, crs):
        self.L, self.h = L, ctypes.c_void_p()
        zk.check(L.zkt_pinocchio_vk_create(ctypes.byref(crs), ctypes.byref(self.h)))
    def __enter__(self): return self
    def __exit__(self, *a): self.L.zkt_pinocchio_vk_free(self.h)
    def verify(self, bufs, io, n, expect=ZKT_OK, room=None):
        """bufs: field -> (n, words) array; io: (n * n_io, 4) array or None; room: verdict words to hand over (n unless given), pre-set to 77"""
        pf = PinProof()
        for k, v in bufs.items(): setattr(pf, k, ptr(v))
        verdict = np.full(n if room is None else room, 77, np.int32)
        rc = self.L.zkt_pinocchio_verify_batch(self.h, ctypes.byref(pf), ptr(io) if io is not None else None, n, verdict.ctypes.data_as(ctypes.c_void_p))
        assert rc == expect, rc
        return [int(v) for v in verdict]


def proof_arrays(L, proofs):
    """model proofs -> the struct of arrays zkt_pinocchio_verify_batch takes, one multiplication call per field"""
    return {field: points(L, [p[k] for p in proofs], field in G2_FIELDS) for k, field in M.PROOF_FIELDS.items()}


def single(L, crs, bufs, i, io_i):
    """zkt_pinocchio_verify on proof i of a batch"""
    pf, pb = alloc_pinocchio_proof()
    for k in pb: pb[k][:] = bufs[k][i]
    return L.zkt_pinocchio_verify(ctypes.byref(crs), ctypes.byref(pf), ptr(io_i) if io_i is not None else None)


def same_outcome(batch, one):
    return batch == one or (batch < 0 and one < 0)          # a panic is a panic, wherever the reference's chain meets it


N_IO = 3
MUTATIONS = [("reject", c) for c in range(5)] + [("panic", c) for c in range(5)] + [("reject-before-panic", 1)]


def mutate(proof, kind, c):
    return M.rejecting_at(proof, c) if kind == "reject" else M.panicking_at(proof, c) if kind == "panic" else M.reject_before_panic(proof)


@pytest.fixture(scope="module")
def keyed(L):
    """one key from exponents with n_io = 3, its handle, and 130 accepting proofs with their statements (shared, never written to)"""
    rng = SplitMix64(20240)
    key = M.random_key(rng, N_IO)
    crs, buf = key_struct(L, key)
    ios = [[1] + [rng.below(R) for _ in range(N_IO - 1)] for _ in range(130)]
    proofs = [M.accepting_proof(key, io, rng) for io in ios]
    with Handle(L, crs) as h:
        yield key, crs, buf, h, ios, proofs


# lanes that carry a mutation: lane 0, the two sides of the first wave boundary, the last element and one more lane of the last partial wave; `first` spreads the eleven
# mutations over the sizes so that every one of them is met
@pytest.mark.parametrize("n,lanes,first", [(1, [0], 0), (2, [0, 1], 1), (63, [0, 31, 62], 3), (64, [0, 32, 63], 6), (65, [0, 63, 64], 9), (130, [0, 63, 64, 128, 129], 1)])
def test_pinocchio_batch_equals_model(L, keyed, n, lanes, first):
    key, crs, buf, h, ios, proofs = keyed
    batch = [dict(p) for p in proofs[:n]]
    for k, lane in enumerate(lanes):
        kind, c = MUTATIONS[(first + k) % len(MUTATIONS)]
        batch[lane] = mutate(batch[lane], kind, c)
    want = [M.decide(key, p, io) for p, io in zip(batch, ios)]
    assert all(w == 1 for i, w in enumerate(want) if i not in lanes) and all(want[i] != 1 for i in lanes)
    got = h.verify(proof_arrays(L, batch), ints_to_arr([w for io in ios[:n] for w in io], 4), n)
    assert got == want


def test_pinocchio_batch_covers_every_mutation():
    seen = set()
    for n, lanes, first in [(1, 1, 0), (2, 2, 1), (63, 3, 3), (64, 3, 6), (65, 3, 9), (130, 5, 1)]: seen |= {(first + k) % len(MUTATIONS) for k in range(lanes)}
    assert seen == set(range(len(MUTATIONS)))


@pytest.mark.parametrize("case", ["cubic", "chain4"])
def test_pinocchio_batch_equals_single_call_on_real_instances(L, case):
    """eight copies of one real proof with the mutations of test_pinocchio_vs_oracle: verdict[i] is what zkt_pinocchio_verify returns for proof i"""
    A, B, C, wit, l = example_cubic() if case == "cubic" else chain_circuit(4)
    n_c, n_io = len(A), l + 1
    V, W, Y, hq, max_degree = pinocchio_instance(A, B, C, wit)
    rng = SplitMix64(977 + n_c)
    rnd = ints_to_arr([rng.below(R - 1) + 1 for _ in range(8)], 4)
    dv, dy = ints_to_arr([rng.below(R - 1) + 1], 4), ints_to_arr([rng.below(R - 1) + 1], 4)
    wires, H = ints_to_arr(wit, 4), ints_to_arr(hq, 4)
    crs, cbuf = alloc_pinocchio(n_c, n_io, len(wit) - n_io, max_degree)
    zk.check(L.zkt_pinocchio_setup(ctypes.byref(crs), ptr(V), ptr(W), ptr(Y), ptr(rnd)))
    pf, pb = alloc_pinocchio_proof()
    zk.check(L.zkt_pinocchio_prove(ctypes.byref(crs), ptr(wires), ptr(H), len(hq), ptr(dv), ptr(dy), ctypes.byref(pf)))
    n = 8
    bufs = {k: np.repeat(v, n, axis=0) for k, v in pb.items()}
    io = np.tile(wires[:n_io], (n, 1))
    io[1 * n_io + n_io - 1, 0] ^= np.uint64(1)                                            # 1: bad io, the divisibility check fails
    bufs["alpha_y_mid_s"][2] = bufs["alpha_v_mid_s"][2]                                    # 2: the knowledge-of-coefficient check of y fails
    for i in (3, 4):                                                                       # 3: an argument at infinity in the third check, the second still passes
        bufs["alpha_y_mid_s"][i] = bufs["alpha_v_mid_s"][i]; bufs["g2_w_mid_s"][i] = 0; bufs["g2_w_mid_s"][i, 24] = 1
    bufs["alpha_v_mid_s"][4] = bufs["v_mid_s"][4]                                          # 4: ... but a rejection by the second check wins
    bufs["h_s"][6] = 0; bufs["h_s"][6, 24] = 1                                             # 6: only the last equality has an argument at infinity
    with Handle(L, crs) as h:
        got = h.verify(bufs, io, n)
    one = [single(L, crs, bufs, i, io[i * n_io:(i + 1) * n_io].copy()) for i in range(n)]
    assert got == one
    assert got == [1, 0, 0, -ZKT_ERR_INFINITY, 0, 1, -ZKT_ERR_INFINITY, 1]
    for i in (0, 3):                                                                       # the accepting proof and one panic against the oracle as well
        opf, opb = alloc_pinocchio_proof()
        for k in opb: opb[k][:] = bufs[k][i]
        assert O.zkto_pinocchio_verify(ctypes.byref(crs), ctypes.byref(opf), ptr(io[i * n_io:(i + 1) * n_io].copy())) == (1 if i == 0 else -2)


def outside_their_groups(L, keyed):
    """n = 70, honest except four lanes: each verdict is the single call's outcome for that proof, every neighbour is still 1"""
    key, crs, buf, h, ios, proofs = keyed
    n, rng = 70, SplitMix64(99)
    bufs = proof_arrays(L, proofs[:n])
    io = ints_to_arr([w for q in ios[:n] for w in q], 4)
    deg = dict(degenerate_g1_points())
    bufs["h_s"][0] = g2_arr([to_abi_g2(py_twist_point(rng))])[0]                           # on E', outside G2
    (x1, x0), (y1, y0) = g2_from_arr(bufs["g2_w_mid_s"][63])[0]
    bufs["g2_w_mid_s"][63] = g2_arr([((x1, x0), (y1, (y0 + 1) % Q))])[0]                   # off E'
    bufs["alpha_v_mid_s"][64] = g1_arr([deg["order | 121"]])[0]                            # on E, outside G1
    bufs["y_mid_s"][69] = g1_arr([deg["G1 point + cofactor point"]])[0]
    got = h.verify(bufs, io, n)
    special = (0, 63, 64, 69)
    for i in special:
        one = single(L, crs, bufs, i, io[i * N_IO:(i + 1) * N_IO].copy())
        assert same_outcome(got[i], one), (i, got[i], one)
    assert all(got[i] == 1 for i in range(n) if i not in special)
    return [got[i] for i in special]


def test_pinocchio_batch_points_off_their_groups(L, keyed):
    outside_their_groups(L, keyed)


def test_pinocchio_batch_fail_closed(L, keyed):
    L.zkt_verify_set_fail_closed(1)
    try:
        got = outside_their_groups(L, keyed)
    finally:
        L.zkt_verify_set_fail_closed(0)
    assert got[2] == 0 and got[3] == 0                       # G1 arguments outside the subgroup are rejected, not evaluated


@pytest.mark.parametrize("which", ["gamma", "alpha_w"])
def test_pinocchio_batch_key_off_the_fast_path(L, keyed, which):
    """a key with a point outside its group is still a valid handle; its proofs are decided as the single call decides them"""
    key, _, _, _, ios, proofs = keyed
    crs, buf = key_struct(L, key)
    if which == "gamma": buf["gamma"][:] = g2_arr([to_abi_g2(py_twist_point(SplitMix64(5)))])
    else: buf["alpha_w"][:] = g1_arr([dict(degenerate_g1_points())["generic curve point"]])
    n = 3
    batch = [dict(p) for p in proofs[:n]]
    batch[1] = M.rejecting_at(batch[1], 4)
    bufs = proof_arrays(L, batch)
    io = ints_to_arr([w for q in ios[:n] for w in q], 4)
    with Handle(L, crs) as h:
        got = h.verify(bufs, io, n)
    for i in range(n):
        one = single(L, crs, bufs, i, io[i * N_IO:(i + 1) * N_IO].copy())
        assert same_outcome(got[i], one), (which, i, got[i], one)


@pytest.mark.parametrize("n_io", [0, 1, 12])
def test_pinocchio_batch_io_counts(L, n_io):
    rng = SplitMix64(300 + n_io)
    key = M.random_key(rng, n_io)
    crs, buf = key_struct(L, key)
    ios = [([1] + [rng.below(R) for _ in range(n_io - 1)])[:n_io] for _ in range(2)] + [[0] * n_io]      # the last statement is all zero
    batch = [M.accepting_proof(key, io, rng) for io in ios]
    batch[1] = M.rejecting_at(batch[1], 4)
    want = [M.decide(key, p, io) for p, io in zip(batch, ios)]
    assert want == [1, 0, 1]
    bufs = proof_arrays(L, batch)
    flat = [w for io in ios for w in io]
    with Handle(L, crs) as h:
        assert h.verify(bufs, ints_to_arr(flat, 4) if n_io else None, 3) == want
        if n_io:                                             # a wire plus r is used as the integer it is: the same exponent
            big = list(flat); big[n_io - 1] += R
            assert h.verify(bufs, ints_to_arr(big, 4), 3) == want
            assert h.verify(bufs, None, 3, expect=ZKT_ERR_SHAPE) == [77] * 3


def test_pinocchio_batch_shapes_and_handles(L, keyed):
    key, crs, buf, h, ios, proofs = keyed
    crs13, keep13 = alloc_pinocchio(4, 13, 1, 1)
    for k in buf:
        if buf[k].shape[0] == 1: setattr(crs13, k, ptr(buf[k]))
    bad = ctypes.c_void_p()
    assert L.zkt_pinocchio_vk_create(ctypes.byref(crs13), ctypes.byref(bad)) == ZKT_ERR_SHAPE and not bad.value
    assert L.zkt_pinocchio_vk_create(ctypes.byref(crs), None) == ZKT_ERR_SHAPE
    n = 2
    bufs = proof_arrays(L, proofs[:n]); io = ints_to_arr([w for q in ios[:n] for w in q], 4)
    assert h.verify(bufs, io, 0, room=2) == [77, 77]                                               # n = 0: ZKT_OK, nothing written
    pf = PinProof()
    for k, v in bufs.items(): setattr(pf, k, ptr(v))
    assert L.zkt_pinocchio_verify_batch(h.h, ctypes.byref(pf), ptr(io), n, None) == ZKT_ERR_SHAPE
    # two handles used alternately; a handle freed and another created
    rng = SplitMix64(8)
    key2 = M.random_key(rng, N_IO)
    crs2, buf2 = key_struct(L, key2)                     # buf2 owns the memory crs2 points to
    proofs2 = [M.accepting_proof(key2, q, rng) for q in ios[:n]]
    bufs2 = proof_arrays(L, proofs2)
    with Handle(L, crs2) as h2:
        for rep in range(2):
            assert h.verify(bufs, io, n) == [1, 1] and h2.verify(bufs2, io, n) == [1, 1]
        assert h2.verify(bufs, io, n) == [M.decide(key2, p, q) for p, q in zip(proofs[:n], ios)] == [0, 0]
    with Handle(L, crs2) as h3:
        assert h3.verify(bufs2, io, n) == [1, 1] and h.verify(bufs, io, n) == [1, 1]


def test_pinocchio_batch_one_proof_per_lane_kernels_in_a_forced_process():
    """With ZKT_DPRODUCT_MAX = 0 the small-batch kernels refuse, so every n above takes k_pinocchio_check and the large form of the launchers behind it: the module once
    more in ONE child process (which deselects this test: no grandchild)."""
    env = dict(os.environ, ZKT_DPRODUCT_MAX="0", ZKT_DTATE_MAX="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "not forced_process", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout


def test_pinocchio_batch_in_two_pieces_in_a_forced_process():
    """A batch just above what the lane-distributed launcher takes in one call is verified in two pieces (zkt_pinocchio_verify_batch).  With ZKT_DPRODUCT_MAX = 600 a
    piece is 40 proofs: n = 63, 64, 65 of the model test go in two pieces with a mutated lane in each, n = 130 to the one-proof-per-lane kernels, n = 1, 2 in one piece."""
    env = dict(os.environ, ZKT_DPRODUCT_MAX="600")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "equals_model", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout and "skipped" not in r.stdout
