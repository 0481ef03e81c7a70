"""One rank of the world-3 / world-8 rehearsal of the exchange and the combine on exceptional shards (include/zkt.h "multi-GPU", csrc/zkt_comm.cpp): launched by
tests/test_gpu_comm.py, `world` processes sharing ONE card, the callback transport over gloo as in tests/comm_worker.py.

For G1, G2 and secp256k1: an empty last shard, an uneven split, the same point on every rank (every tree addition of the combine a doubling), ranks that cancel,
all-zero scalars, three MSMs in flight collected through the exchange, a rank whose local stage fails, a failing all-gather callback; then sharded Groth16 proofs
with one constraint per rank.  Every expected value comes from python integers.

The worker never strands its peers: every rank makes the same fixed sequence of collective calls whatever it observes (a local step that fails leaves a NULL handle,
and the collective call is made with it), mismatches are collected and reported at the end.  Prints `COMM_CASES_OK <rank>`, or the mismatches and exit status 1."""
import ctypes, importlib, os, sys, traceback
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from zkt_testlib import ptr, SplitMix64, R, G1W, G2W, SECP_N, ints_to_arr
    from test_gpu_combine import _point, GEN
    zk = importlib.import_module("zk-toolkit_amd")
    zk.init(0)
    L = zk.lib()
    bad = []
    fail_next = [False]

    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)

    def allgather(_ctx, send, recv, nbytes):
        try:
            if fail_next[0]:                                     # case 8: every rank fails this one call, none gathers
                fail_next[0] = False
                return 1
            mine = torch.frombuffer((ctypes.c_uint8 * nbytes).from_address(send), dtype=torch.uint8).clone()
            parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(parts, mine)
            buf = torch.cat(parts).numpy()
            ctypes.memmove(recv, buf.ctypes.data, nbytes * world)
            return 0
        except Exception as e:       # never let an exception cross the C boundary
            print("allgather callback failed:", repr(e), flush=True)
            return 1
    cb = CB(allgather)
    zk.check(L.zkt_comm_init_callback(rank, world, ctypes.cast(cb, ctypes.c_void_p), None))
    assert L.zkt_comm_rank() == rank and L.zkt_comm_world() == world

    W = {"g1": G1W, "g2": G2W, "secp": 9}
    ORDER = {"g1": R, "g2": R, "secp": SECP_N}
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    fn = lambda group, name: getattr(L, f"zkt_{group}_{name}")

    class Shard:
        """this rank's resident bases k_i * G and device scalars; a local failure leaves h = None, which the collective calls pass on as a NULL handle"""
        def __init__(self, group, ks, ss):
            self.group, self.n, self.h, self.d_s = group, len(ks), None, None
            try:
                host = np.zeros((max(self.n, 1), W[group]), np.uint64)
                if self.n:
                    zk.check(fn(group, "mul_batch")(ptr(np.repeat(GEN[group], self.n, axis=0)), ptr(ints_to_arr(ks, 4)), 4, ptr(host), self.n))
                    self.d_s = torch.from_numpy(ints_to_arr(ss, 4).view(np.int64)).cuda()
                h = ctypes.c_void_p()
                zk.check(fn(group, "bases_upload")(ptr(host) if self.n else None, self.n, ctypes.byref(h)))
                self.h = h
            except Exception:
                bad.append(f"{group}: building a shard of {self.n} terms failed on rank {rank}:\n{traceback.format_exc()}")

        def sharded(self, handle="own", scalars="own"):
            """COLLECTIVE: (status, point)"""
            got = np.full((1, W[self.group]), 0x5A5A5A5A5A5A5A5A, np.uint64)
            rc = fn(self.group, "msm_sharded")(self.h if handle == "own" else handle, vp(self.d_s if scalars == "own" else scalars), ctypes.c_size_t(self.n), None, ptr(got))
            return rc, got

        def submit(self, slot):
            try:
                zk.check(fn(self.group, "msm_submit")(self.h, vp(self.d_s), self.n, None, slot))
            except Exception as e:
                bad.append(f"{self.group}: submit on slot {slot} failed on rank {rank}: {e!r}")

        def collect(self, slot):
            """COLLECTIVE: (status, point)"""
            got = np.full((1, W[self.group]), 0x5A5A5A5A5A5A5A5A, np.uint64)
            return fn(self.group, "msm_sharded_collect")(self.h, slot, ptr(got)), got

        def free(self):
            if self.h is not None:
                fn(self.group, "bases_free")(self.h)

    def expect(what, res, tot, status=0):
        rc, got = res
        if rc != status:
            bad.append(f"{what}: status {rc} on rank {rank}, expected {status}")
        elif status == 0 and not (got == _point(what.split()[0], tot)).all():
            bad.append(f"{what}: the point on rank {rank} differs from python integers")
        elif status != 0 and not (got == 0x5A5A5A5A5A5A5A5A).all():
            bad.append(f"{what}: the output was written although the call returned {rc} (rank {rank})")

    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()

    def my_range(n):
        L.zkt_comm_shard_range(ctypes.c_size_t(n), rank, world, ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    for gi, group in enumerate(("g1", "g2", "secp")):
        order = ORDER[group]
        rng = SplitMix64(0xC0 + gi)                              # every rank draws the same global problems
        below = lambda: rng.below(order - 1) + 1

        # 1. empty last shard: world - 1 terms, the last rank holds none
        n = world - 1
        ks, ss = [below() for _ in range(n)], [below() for _ in range(n)]
        a, b = my_range(n)
        if rank == world - 1 and b - a != 0:
            bad.append(f"{group}: the last rank of {n} terms over {world} ranks holds {b - a} terms")
        empty = Shard(group, ks[a:b], ss[a:b])
        expect(f"{group} empty last shard", empty.sharded(), sum(k * s for k, s in zip(ks, ss)) % order)

        # 2. uneven split: 8 world + 1 terms
        n = 8 * world + 1
        ks, ss = [below() for _ in range(n)], [below() for _ in range(n)]
        a, b = my_range(n)
        uneven, tot2 = Shard(group, ks[a:b], ss[a:b]), sum(k * s for k, s in zip(ks, ss)) % order
        expect(f"{group} uneven split", uneven.sharded(), tot2)

        # 3. the same point c * G on every rank, from rank-dependent (k, s): two terms G and k_r G with s_0 = c - k_r s_1
        c = below()
        per_rank = [(below(), below()) for _ in range(world)]
        kr, s1 = per_rank[rank]
        same, tot3 = Shard(group, [1, kr], [(c - kr * s1) % order, s1]), world * c % order
        expect(f"{group} same point on every rank", same.sharded(), tot3)

        # 4. ranks r and r ^ 1 cancel; in an odd world the last rank's point is left over
        pairs = [(below(), below(), below()) for _ in range((world + 1) // 2)]          # (c_j, k_j, s_1j)
        cj, kj, sj = pairs[rank >> 1]
        s = [(cj - kj * sj) % order, sj]
        if rank & 1:
            s = [(order - x) % order for x in s]
        cancel, tot4 = Shard(group, [1, kj], s), (pairs[-1][0] if world & 1 else 0)
        expect(f"{group} cancelling ranks", cancel.sharded(), tot4)

        # 5. all zero: every rank's scalars are zero
        zero = torch.zeros((max(uneven.n, 1), 4), dtype=torch.int64, device="cuda")
        expect(f"{group} all-zero scalars", uneven.sharded(scalars=zero), 0)

        # 6. pipelined: cases 2, 3, 4 in flight on slots 0, 1, 2, collected through the exchange in that order
        for slot, sh in enumerate((uneven, same, cancel)):
            sh.submit(slot)
        for slot, (sh, tot) in enumerate(((uneven, tot2), (same, tot3), (cancel, tot4))):
            expect(f"{group} pipelined slot {slot}", sh.collect(slot), tot)

        # 7. a failing rank: the last rank passes a NULL handle; every rank returns ZKT_ERR_SHAPE, zkt_last_error_index keeps its value, the communicator survives
        if group == "g1":
            before = L.zkt_last_error_index()
            expect("g1 NULL handle on the last rank", uneven.sharded(handle=None if rank == world - 1 else "own"), None, status=zk.ZKT_ERR_SHAPE)
            if L.zkt_last_error_index() != before:
                bad.append(f"g1 NULL handle on the last rank: zkt_last_error_index changed from {before} to {L.zkt_last_error_index()} on rank {rank}")
            expect("g1 uneven split after the failing rank", uneven.sharded(), tot2)

        # 8. a failing callback: every rank's callback returns 1 for one call without gathering -> ZKT_ERR_DEVICE everywhere, and the next call is served
        fail_next[0] = True
        expect(f"{group} failing callback", uneven.sharded(), None, status=zk.ZKT_ERR_DEVICE)
        if fail_next[0]:
            bad.append(f"{group} failing callback: the callback was not called on rank {rank}")
            fail_next[0] = False
        expect(f"{group} uneven split after the failing callback", uneven.sharded(), tot2)

        for sh in (empty, uneven, same, cancel):
            sh.free()

    # 9. sharded Groth16 proofs against the python-integer proof: one constraint per rank (the C2 range is empty on some ranks), and 200 constraints at world 3
    from test_gpu_r1cs_plans import _inputs, _points, _setup, _new
    from qap_util import asym_circuit_sparse, groth16_proof_scalars
    for n in [world] + ([200] if world == 3 else []):
        mats, wires, l, m = asym_circuit_sparse(n, seed=4000 + n)
        trap, rs = _inputs(n)
        want = _points(*groth16_proof_scalars(mats, wires, l, trap, *rs[0]))
        pk, d_w = None, None
        try:
            rc, vbuf, pk = _setup(L, mats, n, l, m, trap, rank, world)
            zk.check(rc)
            d_w = torch.from_numpy(wires.view(np.int64)).cuda()
        except Exception:
            bad.append(f"groth16 n = {n}: the key of rank {rank} failed:\n{traceback.format_exc()}")
            pk = None
        got = _new()
        rc = L.zkt_groth16_prove_r1cs_sharded(pk, d_w.data_ptr() if d_w is not None else None, rs[0][0].ctypes.data, rs[0][1].ctypes.data,
                                              *[x.ctypes.data for x in got])              # COLLECTIVE
        if rc != 0:
            bad.append(f"groth16 n = {n}: status {rc} on rank {rank}")
        else:
            bad.extend(f"groth16 n = {n}: proof element {nm} on rank {rank} differs from python integers" for g, w, nm in zip(got, want, "ABC") if not (g == w).all())
        if pk:
            L.zkt_groth16_pk_free(pk)

    L.zkt_comm_finalize()
    dist.barrier()
    dist.destroy_process_group()
    if bad:
        print(f"COMM_CASES_MISMATCH rank {rank}: {len(bad)}", flush=True)
        for line in bad:
            print("  " + line, flush=True)
        sys.exit(1)
    print(f"COMM_CASES_OK {rank}", flush=True)


if __name__ == "__main__":
    main()
