"""Stream ordering of every device-pointer entry point of include/zkt.h and of the resident MSM handle's pipeline.

INTEGRATION.md: "entry points that take a `stream` argument order their work behind it".  Arithmetic tests cannot see that promise broken, so every
case here is a DELAYED PRODUCER: the input buffer holds a valid input A (written and synchronised on the default stream); on a non-blocking stream of
the caller's a delay is enqueued and behind it a device-side copy of another valid input B into the same buffer; then the library is called with that
stream.  The result must be the python-integer value for B.  A and B are both well formed, so a lost wait gives A's answer — a wrong value, no fault.

  delay        torch.cuda._sleep, calibrated once per module with events (a chain of additions on a 256 MB tensor if _sleep fails on the device).
  warm-up      before every delayed call the same call runs on the NULL stream with input A (slot buffers, graph capture, twiddle and comb tables);
               the host time of that warmed call is measured, and the delay is never less than 20 times the slowest one seen so far, nor below 20 ms:
               a delay 20 times the slowest warmed call cannot have run out before that call returns.
  in effect    every delayed call proves that its delay was still running: an event recorded behind the copy of B is unfinished when a call that only
               enqueues returns; a blocking call takes at least half the delay.  A case that cannot show it fails with "delay ineffective".
  streams      a caller stream that shares a hardware queue with the library's stream is ordered by the queue alone, so every case runs from
               GPU_MAX_HW_QUEUES + 1 caller streams (default 4 + 1), created one after another.
  results      a call that leaves its result on the caller's stream is read by a clone() enqueued on that stream, with no host synchronisation in
               between; output buffers start as a pattern and carry a guard row.

tests/stream_order_model.py maps every `void* stream` function of the header to its case here (or to the reason it has none) and restates the constants
of zkt_msm_handle.cpp the pipeline cases use; tests/test_stream_order_model.py checks both on the CPU.

Measured on an MI355X with GPU_MAX_HW_QUEUES=4 (the fixture prints both figures; five runs): the slowest warmed call is zkt_g2_bases_from_device of 65 points
at 6.2 to 7.9 ms of host time, so the delay was 124 to 159 ms; torch.cuda._sleep worked and calibrated to 2.39e6 units per millisecond.
Streams and queues, as observed: with the input wait of msm_submit taken out of a scratch build, the call read the stale input A from every one of twelve
caller streams created one after another, for slots 0, 1 and 7 alike; no caller stream was ordered behind the handle's reduce stream by a shared hardware
queue.  (The handle's reduce streams are high-priority and torch's are not; whether that is why has not been measured.)  Each of the three waits named in
stream_order_model.SOURCE_LINES, taken out alone, turned its cases red through a wrong value on the first caller stream."""
import contextlib, ctypes, importlib, os, subprocess, sys, threading, time
import numpy as np
import pytest
import msm_plan_model as M
import stream_order_model as S
from zkt_testlib import (Q, G1W, G2W, G1_GEN, G2_GEN, SECP_GEN, SplitMix64, py_g1_mul, py_g2_mul, py_secp_mul, g1_arr, g2_arr, secp_arr, to_abi_g2,
                         ints_to_arr, ptr)

pytestmark = pytest.mark.gpu
if os.environ.get("ZKT_MSM_C"):
    pytest.skip("a forced window width changes which set takes the three-stream branch", allow_module_level=True)
zk = importlib.import_module("zk-toolkit_amd")

CHILD_ENV = "ZKT_STREAM_ORDER_CHILD"                                  # set in the child process of the launch-by-launch test
NCALLER = int(os.environ.get("GPU_MAX_HW_QUEUES") or 4) + 1          # caller streams per case
N_LANES = 65                                                          # one wave and one lane
N_MSM = 300
N_SMALL = 700
N_LARGE = 1 << S.LARGE_LOG2
DELAY_FLOOR_MS, DELAY_FACTOR, DELAY_CAP_MS = 20.0, 20.0, 1500.0
PATTERN64, PATTERN32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
W = {"g1": G1W, "g2": G2W, "secp": 9}
PW = {"g1": zk.G1_PARTIAL_WORDS, "g2": zk.G2_PARTIAL_WORDS, "secp": zk.SECP_PARTIAL_WORDS}
GEN = {"g1": g1_arr([G1_GEN]), "g2": g2_arr([G2_GEN]), "secp": secp_arr([SECP_GEN])}


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _sp(st):
    return ctypes.c_void_p(st.cuda_stream) if st is not None else None


def _sz(n):
    return ctypes.c_size_t(n)


def _fn(L, group, name):
    return getattr(L, f"zkt_{group}_{name}")


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def _guarded(want, pattern):
    """the expected contents of an output buffer of len(want) + 1 rows that started as `pattern`"""
    want = np.asarray(want)
    return np.concatenate([want, np.full((1,) + want.shape[1:], pattern, want.dtype)])


def _point(group, tot):
    if group == "g1":
        return g1_arr([py_g1_mul(G1_GEN, tot)])
    if group == "secp":
        return secp_arr([py_secp_mul(SECP_GEN, tot)])
    (x1, x0), (y1, y0) = G2_GEN
    pt = py_g2_mul(((x0, x1), (y0, y1)), tot)
    return g2_arr([None if pt is None else to_abi_g2(pt)])


def _rand256(seed, n):
    """n 254-bit values as (n, 4) uint64 (scalars are used as-is, so no reduction is needed)"""
    k = np.random.Generator(np.random.PCG64(seed)).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    k[:, 3] >>= np.uint64(2)
    return k


def _host_out(group, rows=1):
    """a host output buffer for `rows` points: a pattern, and one row more than the call may write"""
    return np.full((rows + 1, W[group]), PATTERN64, np.uint64)


def _unguard(got):
    """the rows of a _host_out buffer the call owns; the guard row must still hold the pattern"""
    assert (got[-1] == PATTERN64).all(), "the call wrote past its host output"
    return got[:-1]


def _dot(kint, scalars, group):
    return sum(k * s for k, s in zip(kint, M.ints_from_scalars(scalars))) % M.ORDER[group]


# ---- the harness -------------------------------------------------------------------------------------------------------------------------
class Harness:
    def __init__(self, L):
        import torch
        self.L = L
        self.streams = [torch.cuda.Stream() for _ in range(max(NCALLER, S.MSM_SLOTS + 1))]      # non-blocking (torch creates its streams so), one after another
        self.delay_ms, self.slowest_ms, self.slowest_name = DELAY_FLOOR_MS, 0.0, "none"
        self.last_call_s = 0.0
        self._calibrate()

    # -- the delay: spin cycles per millisecond, or additions on a large tensor per millisecond
    def _timed_ms(self, fn):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    def _calibrate(self):
        import torch
        try:
            cycles = 1 << 20
            torch.cuda._sleep(cycles); torch.cuda.synchronize()
            ms = self._timed_ms(lambda: torch.cuda._sleep(cycles))
            while ms < 5.0 and cycles < 1 << 40:
                cycles <<= 2
                ms = self._timed_ms(lambda: torch.cuda._sleep(cycles))
            self.mode, self.per_ms, self.big = "_sleep", cycles / ms, None
        except (RuntimeError, AttributeError):
            self.big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
            def chain(k):
                for _ in range(k): self.big.add_(1.0)
            chain(4); torch.cuda.synchronize()
            self.mode, self.per_ms = "add chain", 32 / self._timed_ms(lambda: chain(32))

    def sleep(self, ms):
        """enqueue a delay of `ms` on the current stream"""
        import torch
        units = int(ms * self.per_ms) + 1
        if self.big is None:
            torch.cuda._sleep(units)
        else:
            for _ in range(units): self.big.add_(1.0)

    # -- calls
    def call(self, fn, *args):
        """a library call, checked; its host time is kept in last_call_s"""
        t0 = time.perf_counter()
        rc = fn(*args)
        self.last_call_s = time.perf_counter() - t0
        zk.check(rc)

    def warmed(self, name, seconds):
        """a warmed call took `seconds` on the host: the delay is at least DELAY_FACTOR times the slowest of them"""
        ms = seconds * 1e3
        if ms > self.slowest_ms:
            self.slowest_ms, self.slowest_name = ms, name
        self.delay_ms = max(self.delay_ms, DELAY_FACTOR * self.slowest_ms)
        assert self.delay_ms <= DELAY_CAP_MS, f"{name}: a warmed call of {ms:.1f} ms asks for a delay of {self.delay_ms:.0f} ms: too slow for a quick test"

    def produce(self, st, pairs, ms=None):
        """on `st`: the delay, then the device-side copies dst <- src; returns an event recorded behind them"""
        import torch
        with torch.cuda.stream(st):
            self.sleep(self.delay_ms if ms is None else ms)
            for dst, src in pairs:
                dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        return ev

    def in_effect(self, what, ev=None, blocking_s=None, delay_ms=None):
        d = self.delay_ms if delay_ms is None else delay_ms
        if ev is not None:
            assert not ev.query(), f"delay ineffective: {what}: the producer of B had finished when the call returned ({d:.0f} ms delay)"
        else:
            assert blocking_s * 1e3 >= d / 2, f"delay ineffective: {what}: the blocking call took {blocking_s * 1e3:.1f} ms under a delay of {d:.0f} ms"

    def report(self, when):
        print(f"\n[stream order] {when}: delay by {self.mode} ({self.per_ms:.0f} units/ms); slowest warmed call {self.slowest_ms:.3f} ms ({self.slowest_name}); "
              f"delay {self.delay_ms:.1f} ms; {NCALLER} caller streams per case")

    def delayed(self, name, bufs, A, B, call, blocking, outs=(), result=None):
        """The pattern, once per caller stream.  bufs / A / B: the input buffers and device copies of their two contents; call(st) makes the library call on st
        (through self.call, so that its host time is known); outs: [(device output buffer, expected contents for B, guard row included)], read by a clone on the
        caller's stream when the call only enqueues; result(st): a host result for B to compare, returns (got, want)."""
        import torch
        for i, st in enumerate(self.streams[:NCALLER]):
            what = f"{name}, caller stream {i}"
            for b, a in zip(bufs, A): b.copy_(a)
            for o, _ in outs: o.fill_(PATTERN64 if o.dtype == torch.int64 else PATTERN32)
            torch.cuda.synchronize()
            for _ in range(2 if i == 0 else 1):                  # the first call of a case may allocate, capture and build tables; the call after it is the warmed one
                call(None)
                dt = self.last_call_s
                torch.cuda.synchronize()
            self.warmed(name, dt)
            for o, _ in outs: o.fill_(PATTERN64 if o.dtype == torch.int64 else PATTERN32)
            torch.cuda.synchronize()
            ev = self.produce(st, list(zip(bufs, B)))
            call(st)
            waiting, took = not ev.query(), self.last_call_s     # looked at as the call returns; asserted after the values, so that a lost wait shows as a wrong value
            if blocking:
                snaps = [o for o, _ in outs]                     # complete on return: read as they are
            else:
                with torch.cuda.stream(st):
                    snaps = [o.clone() for o, _ in outs]         # ordered by the caller's stream alone
            if result is not None:
                got, want = result(st)
                assert (got == want).all(), f"{what}: the result is not the python-integer value for input B"
            for snap, (o, want) in zip(snaps, outs):
                if not blocking: st.synchronize()
                how = "as the blocking call returned" if blocking else "by a clone on the caller's stream"
                assert (_host(snap) == want).all(), f"{what}: the output read {how} is not the python-integer value for input B (guard row included)"
                assert (_host(o) == want).all(), f"{what}: the output buffer is not the python-integer value for input B (guard row included)"
            if blocking:
                self.in_effect(what, blocking_s=took)
            else:
                assert waiting, f"delay ineffective: {what}: the producer of B had finished when the call returned ({self.delay_ms:.0f} ms delay)"
            torch.cuda.synchronize()


@pytest.fixture(scope="module")
def H():
    import torch
    zk.init()
    h = Harness(zk.lib())
    # the two slowest warmed calls of the module, measured before the first case so that the printed delay is the one the cases start from
    # (every case measures its own warmed call as well, and the delay only grows).  The child of the launch-by-launch test computes no pairing.
    if not os.environ.get(CHILD_ENV):
        _probe_tate(h)
    _probe_bases(h)
    h.report("before the first case")
    yield h
    torch.cuda.synchronize()
    h.report("after the last case")
    _bases.clear()


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------
_bases = {}


def _make_points(L, group, ks):
    """k_i * G on the device: through the device form (G1, G2) or the host-pointer batch (secp256k1 has no device form)"""
    import torch
    n = len(ks)
    ks = np.ascontiguousarray(ks)
    if group == "secp":
        host = np.zeros((n, 9), np.uint64)
        zk.check(L.zkt_secp_mul_batch(ptr(np.repeat(GEN["secp"], n, axis=0)), ptr(ks), 4, ptr(host), _sz(n)))
        return _dev(host)
    d_gen, d_k = _dev(np.repeat(GEN[group], n, axis=0)), _dev(ks)
    d_out = torch.empty((n, W[group]), dtype=torch.int64, device="cuda")
    zk.check(_fn(L, group, "mul_batch_dev")(_vp(d_gen), _vp(d_k), 4, _vp(d_out), _sz(n), None))
    torch.cuda.synchronize()
    return d_out


def _base_set(L, group, n):
    """(device points, python-integer logs) of the first n bases k_i * G of msm_plan_model.random_ks; built once per group at the largest size asked for"""
    have = _bases.get(group)
    if have is None or have[0].shape[0] < n:
        ks = M.random_ks(M.K_SEED)[:n]
        _bases[group] = have = (_make_points(L, group, ks), M.ints_from_scalars(ks))
    return have[0][:n], have[1][:n]


@contextlib.contextmanager
def _handle(L, group, d_bases, n, stream=None, timer=None):
    """a resident base set, freed on the way out whatever happens"""
    h = ctypes.c_void_p()
    fn, args = _fn(L, group, "bases_from_device"), (_vp(d_bases), _sz(n), _sp(stream), ctypes.byref(h))
    if timer is not None: timer.call(fn, *args)
    else: zk.check(fn(*args))
    try:
        yield h
    finally:
        _fn(L, group, "bases_free")(h)


def _msm_dev(L, group, h, d_s, n, stream=None, partial=None, want_out=True):
    got = _host_out(group) if want_out else None
    zk.check(_fn(L, group, "msm_dev")(h, _vp(d_s), _sz(n), _sp(stream), ptr(got), partial))
    return _unguard(got) if want_out else None


def _pack(vectors, n, stride):
    """(k * stride, 4) uint64: vector v at row v * stride, a pattern no result may depend on between the vectors"""
    buf = np.full((len(vectors) * stride, 4), 0xDEADBEEFCAFEF00D, np.uint64)
    for v, s in enumerate(vectors):
        buf[v * stride: v * stride + n] = s
    return buf


# ---- section 2: one delayed-producer case per `void* stream` function ---------------------------------------------------------------------
CASES = {}


def case(cid):
    def deco(f):
        assert cid not in CASES
        CASES[cid] = f
        return f
    return deco


@pytest.mark.parametrize("cid", S.case_ids())
def test_delayed_producer(H, cid):
    CASES[cid](H, cid)


@case("fq_mul_batch_dev")
def _case_fq_mul(H, cid):
    import torch
    n, rng = N_LANES, SplitMix64(1001)
    a1, b1, a2, b2 = ([rng.below(Q) for _ in range(n)] for _ in range(4))
    A, B = [_dev(ints_to_arr(a1, 6)), _dev(ints_to_arr(b1, 6))], [_dev(ints_to_arr(a2, 6)), _dev(ints_to_arr(b2, 6))]
    da, db = torch.empty_like(A[0]), torch.empty_like(A[1])
    out = torch.empty((n + 1, 6), dtype=torch.int64, device="cuda")
    want = _guarded(ints_to_arr([x * y % Q for x, y in zip(a2, b2)], 6), PATTERN64)
    H.delayed(cid, [da, db], A, B, lambda st: H.call(H.L.zkt_fq_mul_batch_dev, _vp(da), _vp(db), _vp(out), _sz(n), _sp(st)), False, outs=[(out, want)])


@case("g1_mul_batch_dev")
@case("g2_mul_batch_dev")
def _case_group_mul(H, cid):
    import torch
    group, n = cid[:2], N_LANES
    sa, sb = _rand256(1101, 8), _rand256(1102, 8)                          # eight distinct scalars per input, cycled over the lanes
    lane = np.arange(n) % 8
    pts = {i: _point(group, k)[0] for i, k in enumerate(M.ints_from_scalars(sb))}
    want = _guarded(np.stack([pts[int(i)] for i in lane]), PATTERN64)
    d_gen = _dev(np.repeat(GEN[group], n, axis=0))
    d_k = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    out = torch.empty((n + 1, W[group]), dtype=torch.int64, device="cuda")
    H.delayed(cid, [d_k], [_dev(sa[lane])], [_dev(sb[lane])],
              lambda st: H.call(_fn(H.L, group, "mul_batch_dev"), _vp(d_gen), _vp(d_k), 4, _vp(out), _sz(n), _sp(st)), False, outs=[(out, want)])


_TATE_LOGS = ((0x1234567, 0x89ABCDE), (0x2F00D5EED, 0x3C0FFEE11))            # (a, b) of the A-pair and of the B-pair: P = a G1, Q = b G2


def _tate_inputs():
    import pairing_route_model as PR
    (a1, b1), (a2, b2) = _TATE_LOGS
    rows = lambda a, b: (np.repeat(PR.g1_rows([PR.g1(a)]), N_LANES, axis=0), np.repeat(PR.g2_rows([PR.g2(b)]), N_LANES, axis=0))
    return rows(a1, b1), rows(a2, b2), np.repeat(PR.gt_words(PR.gt(a2 * b2))[None, :], N_LANES, axis=0)


def _probe_tate(H):
    import torch
    (pa, qa), _, _ = _tate_inputs()
    dp, dq = _dev(pa), _dev(qa)
    out = torch.empty((N_LANES + 1, 72), dtype=torch.int64, device="cuda")
    for _ in range(2):
        H.call(H.L.zkt_tate_batch_dev, _vp(dp), _vp(dq), _vp(out), _sz(N_LANES), None)
    H.warmed("tate_batch_dev", H.last_call_s)


@case("tate_batch_dev")
def _case_tate(H, cid):
    import torch
    (pa, qa), (pb, qb), want = _tate_inputs()
    dp, dq = _dev(pa), _dev(qa)
    out = torch.empty((N_LANES + 1, 72), dtype=torch.int64, device="cuda")
    H.delayed(cid, [dp, dq], [_dev(pa), _dev(qa)], [_dev(pb), _dev(qb)],
              lambda st: H.call(H.L.zkt_tate_batch_dev, _vp(dp), _vp(dq), _vp(out), _sz(N_LANES), _sp(st)), True, outs=[(out, _guarded(want, PATTERN64))])


@case("fr_poly_mul_dev")
def _case_poly_mul(H, cid):
    import torch
    import poly_model as PM
    n = 513
    a1, b1, a2, b2 = (_rand256(1200 + i, n) for i in range(4))
    da, db = _dev(a1), _dev(b1)
    out = torch.empty((2 * n - 1 + 1, 4), dtype=torch.int64, device="cuda")
    want = _guarded(M.scalars_from_ints(PM.kron_mul(M.ints_from_scalars(a2), M.ints_from_scalars(b2))), PATTERN64)
    H.delayed(cid, [da, db], [_dev(a1), _dev(b1)], [_dev(a2), _dev(b2)],
              lambda st: H.call(H.L.zkt_fr_poly_mul_dev, _vp(da), n, _vp(db), n, _vp(out), _sp(st)), False, outs=[(out, want)])


@case("ecdsa_verify_digest_batch_dev")
def _case_ecdsa(H, cid):
    import torch
    import ecdsa_model as E
    n, rng = N_LANES, SplitMix64(1301)
    keys = [1 + rng.below(E.N - 1) for _ in range(4)]
    pubs = [E.gen_pub_key(d) for d in keys]
    lanes = []
    for i in range(n):
        z = rng.below(1 << 256).to_bytes(32, "big")
        sg = E.RETRY
        while sg == E.RETRY:
            sg = E.sign(z, keys[i % 4], 1 + rng.below(E.N - 1))
        lanes.append({"z": z, "r": sg[0], "s": sg[1], "Q": pubs[i % 4]})
    spoiled = [dict(c, s=c["s"] ^ 1) if i % 2 else c for i, c in enumerate(lanes)]       # B: every other lane tampered
    want = np.array([E.verify(c["z"], c["r"], c["s"], c["Q"]) for c in spoiled], np.uint32)
    assert all(E.verify(c["z"], c["r"], c["s"], c["Q"]) for c in lanes[:4]) and want[0::2].all() and not want[1::2].any()
    dig, sig_a, pks = E.pack_cases(lanes)
    _, sig_b, _ = E.pack_cases(spoiled)
    d_dig, d_pk, d_sig = _dev(dig), _dev(pks), _dev(sig_a)
    ok = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    H.delayed(cid, [d_sig], [_dev(sig_a)], [_dev(sig_b)],
              lambda st: H.call(H.L.zkt_ecdsa_verify_digest_batch_dev, d_dig.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), n, ok.data_ptr(), _sp(st)), False,
              outs=[(ok, _guarded(want, PATTERN32))])


@case("ed25519_verify_batch_dev")
def _case_ed25519(H, cid):
    import torch
    import ed25519_model as E
    n, rng = N_LANES, E._Rng(1401)
    keys = [rng.bytes(32) for _ in range(4)]
    pubs = [E.gen_pub_key(k) for k in keys]
    msgs = [rng.bytes(E.MSG_LENGTHS[i % len(E.MSG_LENGTHS)]) for i in range(n)]
    sig_a = [E.sign(m, keys[i % 4]) for i, m in enumerate(msgs)]
    flip = lambda s: s[:40] + bytes([s[40] ^ 1]) + s[41:]                              # a bit of S
    sig_b = [flip(s) if i % 2 else s for i, s in enumerate(sig_a)]                       # B: every other lane tampered
    want = np.array([E.verify(s, pubs[i % 4], msgs[i]) for i, s in enumerate(sig_b)], np.uint32)
    assert all(E.verify(sig_a[i], pubs[i], msgs[i]) for i in range(4)) and want[0::2].all() and not want[1::2].any()
    buf, off = E.pack_messages(msgs)
    to_u8 = lambda xs, w: np.frombuffer(b"".join(xs), dtype=np.uint8).reshape(-1, w).copy()
    d_buf, d_off, d_pub, d_sig = _dev(buf), _dev(off), _dev(to_u8([pubs[i % 4] for i in range(n)], 32)), _dev(to_u8(sig_a, 64))
    ok = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    H.delayed(cid, [d_sig], [_dev(to_u8(sig_a, 64))], [_dev(to_u8(sig_b, 64))],
              lambda st: H.call(H.L.zkt_ed25519_verify_batch_dev, d_buf.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), d_pub.data_ptr(), n, ok.data_ptr(), _sp(st)),
              False, outs=[(ok, _guarded(want, PATTERN32))])


def _probe_bases(H):
    d, _ = _base_set(H.L, "g2", N_LANES)
    for _ in range(2):
        with _handle(H.L, "g2", d, N_LANES, timer=H):
            dt = H.last_call_s
    H.warmed("g2_bases_from_device", dt)


@case("g1_bases_from_device")
@case("g2_bases_from_device")
@case("secp_bases_from_device")
def _case_bases_from_device(H, cid):
    """bases A, then B, in the buffer the handle is built from; afterwards one msm_dev over the handle"""
    import torch
    group, n, L = cid.split("_")[0], N_LANES, H.L
    ka, kb = _rand256(1501, n), _rand256(1502, n)
    pa, pb = _make_points(L, group, ka), _make_points(L, group, kb)
    buf = torch.empty_like(pa)
    s = _rand256(1503, n)
    d_s = _dev(s)
    want = _point(group, _dot(M.ints_from_scalars(kb), s, group))
    got = [None]

    def call(st):
        with _handle(L, group, buf, n, stream=st, timer=H) as h:
            dt = H.last_call_s
            got[0] = _msm_dev(L, group, h, d_s, n)
        H.last_call_s = dt                                                              # the time of zkt_*_bases_from_device alone

    H.delayed(cid, [buf], [pa], [pb], call, True, result=lambda st: (got[0], want))


@case("g1_jac_sum_dev")
@case("g2_jac_sum_dev")
@case("secp_jac_sum_dev")
def _case_jac_sum(H, cid):
    """three Jacobian partials of known sums (msm_collect's dev_partial_jac, through msm_dev), A and B, summed by the call"""
    import torch
    group, n, L, count = cid.split("_")[0], N_LANES, H.L, 3
    d_bases, kint = _base_set(L, group, n)
    parts = {}
    with _handle(L, group, d_bases, n) as h:
        for name, seed in (("A", 1600), ("B", 1610)):
            vecs = [_rand256(seed + j, n) for j in range(count)]
            p = torch.zeros((count, PW[group]), dtype=torch.int32, device="cuda")
            for j, v in enumerate(vecs):
                _msm_dev(L, group, h, _dev(v), n, partial=ctypes.c_void_p(p[j].data_ptr()), want_out=False)
            parts[name] = (p, sum(_dot(kint, v, group) for v in vecs) % M.ORDER[group])
        torch.cuda.synchronize()
    buf = torch.empty_like(parts["A"][0])
    want, got = _point(group, parts["B"][1]), _host_out(group)
    assert parts["A"][1] != parts["B"][1]
    H.delayed(cid, [buf], [parts["A"][0]], [parts["B"][0]],
              lambda st: H.call(_fn(L, group, "jac_sum_dev"), _vp(buf), _sz(count), _sp(st), ptr(got)), True, result=lambda st: (_unguard(got), want))


def _msm_case(H, cid, form):
    """the scalars are the delayed input of a resident set of N_MSM bases; every caller stream takes another slot (submit) so that every reduce stream of the
    handle meets a caller stream"""
    import torch
    group, n, L = cid.split("_")[0], N_MSM, H.L
    d_bases, kint = _base_set(L, group, n)
    if form in ("msm_dev", "msm_submit"):
        sa, sb = _rand256(1700, n), _rand256(1701, n)
        A, B, want = _dev(sa), _dev(sb), _point(group, _dot(kint, sb, group))
    else:
        k, stride = 3, n + 3
        va, vb = [_rand256(1710 + v, n) for v in range(k)], [_rand256(1720 + v, n) for v in range(k)]
        A, B = _dev(_pack(va, n, stride)), _dev(_pack(vb, n, stride))
        want = np.concatenate([_point(group, _dot(kint, v, group)) for v in vb])
    buf = torch.empty_like(A)
    got = _host_out(group, len(want))
    turn = [0]
    with _handle(L, group, d_bases, n) as h:
        def call(st):
            got[:] = PATTERN64
            if form == "msm_dev":
                H.call(_fn(L, group, "msm_dev"), h, _vp(buf), _sz(n), _sp(st), ptr(got), None)
            elif form == "msm_batch_dev":
                H.call(_fn(L, group, "msm_batch_dev"), h, _vp(buf), n, k, stride, _sp(st), ptr(got), None)
            elif form == "msm_batch_submit":
                H.call(_fn(L, group, "msm_batch_submit"), h, _vp(buf), n, k, stride, _sp(st))
            else:
                H.call(_fn(L, group, "msm_submit"), h, _vp(buf), n, _sp(st), 3 * turn[0] % S.MSM_SLOTS)

        def result(st):
            if form == "msm_batch_submit":
                zk.check(_fn(L, group, "msm_batch_collect")(h, ptr(got), None))
            elif form == "msm_submit":
                zk.check(_fn(L, group, "msm_collect")(h, 3 * turn[0] % S.MSM_SLOTS, ptr(got), None))
                if st is not None: turn[0] += 1                                        # the next caller stream takes another slot (warmed there first)
            return _unguard(got), want

        def warm(st):                                                                  # on the NULL stream the submitting forms are collected at once
            call(st)
            if st is None and form.endswith("submit"):
                dt = H.last_call_s
                result(st)
                H.last_call_s = dt

        H.delayed(cid, [buf], [A], [B], warm, form.endswith("_dev"), result=result)


@case("g1_msm_dev")
@case("g2_msm_dev")
@case("secp_msm_dev")
def _case_msm_dev(H, cid): _msm_case(H, cid, "msm_dev")


@case("g1_msm_submit")
@case("g2_msm_submit")
@case("secp_msm_submit")
def _case_msm_submit(H, cid): _msm_case(H, cid, "msm_submit")


@case("g1_msm_batch_submit")
@case("g2_msm_batch_submit")
@case("secp_msm_batch_submit")
def _case_msm_batch_submit(H, cid): _msm_case(H, cid, "msm_batch_submit")


@case("g1_msm_batch_dev")
@case("g2_msm_batch_dev")
@case("secp_msm_batch_dev")
def _case_msm_batch_dev(H, cid): _msm_case(H, cid, "msm_batch_dev")


# ---- section 3: the handle's pipeline under caller streams ------------------------------------------------------------------------------------
def _collect(L, group, h, slot):
    got = _host_out(group)
    zk.check(_fn(L, group, "msm_collect")(h, slot, ptr(got), None))
    return _unguard(got)


@pytest.mark.parametrize("group", S.GROUPS)
def test_small_path_all_slots_in_flight(H, group):
    """n = 700: all eight slots in flight, each fed from its own caller stream behind a delay that is longer the lower the slot (inputs become ready in reverse slot
    order), eight distinct vectors, collected in a shuffled order, and a batch of three in flight on a ninth stream; then a second round rewrites every buffer in
    place on its stream behind a delay, which replays the graphs the first round's addresses are cached under."""
    import torch
    L, n, ns, k = H.L, N_SMALL, S.MSM_SLOTS, 3
    assert not S.large(n) and len(H.streams) >= ns + 1
    d_bases, kint = _base_set(L, group, n)
    rounds = [[_rand256(2000 + 100 * r + j, n) for j in range(ns)] for r in range(3)]            # round 0 is input A of every slot
    batches = [[_rand256(2500 + 100 * r + v, n) for v in range(k)] for r in range(3)]
    want = [[_point(group, _dot(kint, v, group)) for v in vs] for vs in rounds]
    want_b = [np.concatenate([_point(group, _dot(kint, v, group)) for v in vs]) for vs in batches]
    assert len({w.tobytes() for ws in want for w in ws}) == 3 * ns
    d_in = [[_dev(v) for v in vs] for vs in rounds]
    d_in_b = [_dev(_pack(vs, n, n)) for vs in batches]
    d_s = [t.clone() for t in d_in[0]]
    d_b = d_in_b[0].clone()
    torch.cuda.synchronize()
    got_g = _host_out(group, k)
    got_b = got_g[:k]
    with _handle(L, group, d_bases, n) as h:
        for j in range(ns):                                                                     # warm-up on the NULL stream: slot buffers, the graph of (slot, address)
            zk.check(_fn(L, group, "msm_submit")(h, _vp(d_s[j]), _sz(n), None, j))
        for j in range(ns):
            assert (_collect(L, group, h, j) == want[0][j]).all(), f"{group} slot {j}: NULL-stream result"
        zk.check(_fn(L, group, "msm_batch_dev")(h, _vp(d_b), n, k, n, None, ptr(got_b), None))
        assert (got_b == want_b[0]).all()
        for j in range(ns):                                                                     # the warmed calls of this case: a replayed submit, and the batch submit
            H.call(_fn(L, group, "msm_submit"), h, _vp(d_s[j]), _sz(n), None, j); dt = H.last_call_s
            _collect(L, group, h, j); H.warmed(f"{group} msm_submit n={n}", dt)
        H.call(_fn(L, group, "msm_batch_submit"), h, _vp(d_b), n, k, n, None); dt = H.last_call_s
        zk.check(_fn(L, group, "msm_batch_collect")(h, ptr(got_b), None)); H.warmed(f"{group} msm_batch_submit n={n}", dt)
        torch.cuda.synchronize()
        order = np.random.Generator(np.random.PCG64(77)).permutation(ns)
        for r in (1, 2):
            delays = [H.delay_ms * (1 + (ns - 1 - j) / (ns - 1)) for j in range(ns)]           # 2x the delay for slot 0 down to 1x for slot 7
            evs = []
            for j in range(ns):
                evs.append(H.produce(H.streams[j], [(d_s[j], d_in[r][j])], ms=delays[j]))
                zk.check(_fn(L, group, "msm_submit")(h, _vp(d_s[j]), _sz(n), _sp(H.streams[j]), j))
            evs.append(H.produce(H.streams[ns], [(d_b, d_in_b[r])], ms=1.5 * H.delay_ms))
            zk.check(_fn(L, group, "msm_batch_submit")(h, _vp(d_b), n, k, n, _sp(H.streams[ns])))
            for j, ev in enumerate(evs):                                                        # all nine were still waiting when the last call returned
                H.in_effect(f"{group} small path, round {r}, {'slot %d' % j if j < ns else 'batch'}", ev=ev)
            for j in order[::-1] if r == 2 else order:
                assert (_collect(L, group, h, int(j)) == want[r][j]).all(), f"{group} round {r} slot {j}: not the python-integer sum of the vector written behind the delay"
            zk.check(_fn(L, group, "msm_batch_collect")(h, ptr(got_b), None))
            assert (got_b == want_b[r]).all() and (got_g[k] == PATTERN64).all(), f"{group} round {r}: batch"
            torch.cuda.synchronize()


def test_two_host_threads_on_one_handle(H):
    """two threads on disjoint slots of one G1 handle, each with a stream of its own: submit / collect of different slots may come from different threads"""
    import torch
    L, group, n, ns = H.L, "g1", N_SMALL, S.MSM_SLOTS
    d_bases, kint = _base_set(L, group, n)
    rounds = [[_rand256(3000 + 100 * r + j, n) for j in range(ns)] for r in range(3)]
    want = [[_point(group, _dot(kint, v, group)) for v in vs] for vs in rounds]
    d_in = [[_dev(v) for v in vs] for vs in rounds]
    d_s = [t.clone() for t in d_in[0]]
    torch.cuda.synchronize()
    errors = []
    with _handle(L, group, d_bases, n) as h:
        for j in range(ns):                                                                     # warm-up on the NULL stream
            zk.check(_fn(L, group, "msm_submit")(h, _vp(d_s[j]), _sz(n), None, j))
            assert (_collect(L, group, h, j) == want[0][j]).all()
        torch.cuda.synchronize()
        delay = H.delay_ms
        # collect holds the handle's lock while it waits for its slot, so a submit of the other thread issued meanwhile returns only after that wait: both threads
        # submit, look at their events, and meet here before either collects
        gate = threading.Barrier(2, timeout=60)

        def worker(t):
            try:
                st, slots = H.streams[t], range(t * ns // 2, (t + 1) * ns // 2)
                for r in (1, 2):
                    gate.wait()
                    ev = H.produce(st, [(d_s[j], d_in[r][j]) for j in slots], ms=delay)
                    for j in slots:
                        zk.check(_fn(L, group, "msm_submit")(h, _vp(d_s[j]), _sz(n), _sp(st), j))
                    waiting = not ev.query()
                    gate.wait()
                    for j in reversed(slots):
                        if not (_collect(L, group, h, j) == want[r][j]).all():
                            errors.append(f"thread {t}, round {r}, slot {j}: not the python-integer sum of the vector written behind the delay")
                    if not waiting:
                        errors.append(f"delay ineffective: thread {t}, round {r}: the producer had finished when the last submit returned ({delay:.0f} ms delay)")
                    st.synchronize()
            except BaseException as e:                                                         # reported by the main thread
                gate.abort()
                errors.append(f"thread {t}: {type(e).__name__}: {e}")

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
        for t in threads: t.start()
        for t in threads: t.join()
        torch.cuda.synchronize()
    assert not errors, errors


SMALL_PATH_TESTS = "small_path_all_slots or two_host_threads"


def test_launch_by_launch_branch_in_a_child_process():
    """the small-path cases again with ZKT_MSM_GRAPH=0: msm_submit issues the pipeline launch by launch instead of replaying a graph"""
    assert not os.environ.get(CHILD_ENV), "the child runs the small-path tests only"
    env = dict(os.environ, ZKT_MSM_GRAPH="0", **{CHILD_ENV: "1"})
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider", "-k", SMALL_PATH_TESTS],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout, r.stdout[-1000:]


_large_tot = {}


@pytest.mark.parametrize("group", ("g1", "g2"))
def test_large_path_ring_of_twenty(H, group):
    """n = 2^19, the smallest set on the three-stream branch (sort | accumulate | reduce): 20 submits over the 8 slots with five in flight, as bench.py drives the
    handle.  Submit j takes vector j % 3 of three, so a slot never repeats its previous vector and neighbouring slots differ; every result is compared.  Some of the
    submits are delayed producers, one per caller stream: their buffer holds the NEXT vector until the copy behind the delay puts the right one there."""
    import torch
    L, n, ns, steps, depth = H.L, N_LARGE, S.MSM_SLOTS, 20, 5
    assert S.large(n) and not S.large(n - 1)
    d_bases, kint = _base_set(L, group, n)
    vecs = [_rand256(4000 + v, n) for v in range(3)]
    for v in range(3):                                                                          # G1 and G2 have the same order and the same logs: three sums serve both
        if v not in _large_tot:
            _large_tot[v] = _dot(kint, vecs[v], group)
    want = [_point(group, _large_tot[v]) for v in range(3)]
    assert len({w.tobytes() for w in want}) == 3
    d_vec = [_dev(v) for v in vecs]
    nd = min(NCALLER, 7)
    delayed = {6 + 2 * i: i for i in range(nd)}                                                # submit index -> caller stream; each has a buffer of its own
    d_x = {j: d_vec[(j + 1) % 3].clone() for j in delayed}                                      # input A: the next vector
    main = H.streams[-1]
    torch.cuda.synchronize()
    with _handle(L, group, d_bases, n) as h:
        for j in range(ns):                                                                     # warm-up on the NULL stream: every slot's buffers
            zk.check(_fn(L, group, "msm_submit")(h, _vp(d_vec[j % 3]), _sz(n), None, j))
            assert (_collect(L, group, h, j) == want[j % 3]).all(), f"{group} slot {j}: NULL-stream result"
        for j in delayed:                                                                       # and the delayed submits' own path: these are the warmed calls
            H.call(_fn(L, group, "msm_submit"), h, _vp(d_x[j]), _sz(n), None, j % ns); dt = H.last_call_s
            assert (_collect(L, group, h, j % ns) == want[(j + 1) % 3]).all()
            H.warmed(f"{group} msm_submit n=2^19", dt)
        torch.cuda.synchronize()
        for i in range(steps + depth):
            if i >= depth:
                j = i - depth
                assert (_collect(L, group, h, j % ns) == want[j % 3]).all(), f"{group} submit {j} (slot {j % ns}, vector {j % 3}{', delayed' if j in delayed else ''})"
            if i < steps:
                if i in delayed:
                    st = H.streams[delayed[i]]
                    ev = H.produce(st, [(d_x[i], d_vec[i % 3])])
                    zk.check(_fn(L, group, "msm_submit")(h, _vp(d_x[i]), _sz(n), _sp(st), i % ns))
                    H.in_effect(f"{group} large path, submit {i} from caller stream {delayed[i]}", ev=ev)
                else:
                    zk.check(_fn(L, group, "msm_submit")(h, _vp(d_vec[i % 3]), _sz(n), _sp(main), i % ns))
        torch.cuda.synchronize()
