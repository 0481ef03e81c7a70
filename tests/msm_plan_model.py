"""A plain restatement of the MSM's host-side plan and digit scheme (zk-toolkit_amd/csrc/zkt_msm_plan.cpp, msm_sort.h, msm_ws.h), in numpy.

TEST INFRASTRUCTURE.  This is not a simulator of the kernels: it says which window width, task size, sort and merge path a given
scalar vector selects, so that a test can claim "this case reaches branch X" and have the claim checked on the CPU
(tests/test_msm_plan_model.py) before the case runs on the GPU (tests/test_gpu_msm_plans.py).  Whoever retunes the plan tables or the
thresholds below must update this file: test_msm_plan_model.py pins the model to the library's own workspace size."""
import numpy as np

# ---- thresholds, each restating one line of the library -------------------------------------------------------------------------
HOT_NT = 512                # msm_ws.h, `static constexpr uint32_t HOT_NT = 512, HOT_CAP = 64, HOT_FAN = 64;` (k_task_scatter: nt > HOT_NT is hot)
HOT_CAP = 64                # same line: more than HOT_CAP hot buckets and the list is discarded (k_merge_hot returns, k_merge_partials does them all)
HOT_FAN = 64                # same line: blocks per listed hot bucket in k_merge_hot
MERGE_GROUP_MAX = 8         # msm_reduce_coop.h, k_merge_partials `constexpr uint32_t MERGE_GROUP_MAX = 8;` (2..8 pieces: one group; more: the block)
SCATTER_LANE_MAX = 16       # msm_sort.h, k_task_scatter `if (nt <= 16)`: up to 16 tasks written by the bucket's lane, more by the whole block
RED_NG = 16                 # msm_reduce_coop.h, `RED_TPB = 64, RED_NG = RED_TPB / 4`
BULK_MIN = 4 * RED_NG       # msm_reduce_coop.h, coop_block_sum `bulk = count > (size_t)4 * NG` (prime-field groups only: CoopBulk<PrimeOps>)
PART_MIN_ENTRIES = 1 << 22  # msm_sort.h, launch_sort `partition = (size_t)P.nwin * n >= (size_t(1) << 22)`
PART_LO, PART_TPB, PART_CHUNK = 9, 256, 8192       # msm_ws.h, `PART_LO = 9, PART_SUB = 1 << PART_LO, PART_TPB = 256, PART_TILE = 4 * PART_TPB, PART_CHUNK = 8192, PART_MAXP = 2048`
PART_SUB, PART_TILE, PART_MAXP = 1 << PART_LO, 4 * PART_TPB, 2048
GRAPH_MAX_N = 1 << 19       # zkt_msm_handle.cpp, msm_submit `small = h.n < (size_t(1) << 19)`: a small resident set replays a captured graph
CHUNK_MIN, CHUNK_MAX = 8, 128                       # zkt_msm_plan.cpp, pick_chunk: clamp to [8, CHUNK = 128]
TASK_LANES = {"g1": 196608, "secp": 196608, "g2": 65536}   # pick_chunk `tasks = grp == G_G2 ? 65536 : 196608`
COORD_WORDS = {"g1": 14, "g2": 28, "secp": 8}      # msm_ws.h coord_words(): FqC::N = 14 words (zkt_constants.h), Fq2 twice that, SpC::N = 8
GROUPS = ("g1", "g2", "secp")
FORMS = ("resident", "oneshot")

# n on both sides of every step of the plan (resident: msm_plan's width table, the partition threshold at c = 16 and the graph limit;
# one-shot: msm_plan_direct's width c = floor(log2 n) - 3 in [9, 16] and the partition threshold at c = 14)
RESIDENT_STEPS = (1023, 1024, 2047, 2048, 16383, 16384, 246723, 246724, (1 << 19) - 1, 1 << 19)
ONESHOT_STEPS = (8191, 8192, 16383, 16384, 32767, 32768, 65535, 65536, 131071, 131072, 220752, 220753, 262143, 262144, (1 << 19) - 1, 1 << 19)


def _lg(n):
    return max(int(n), 1).bit_length() - 1                               # floor(log2 n), n = 0 counted as 1


def pick_chunk(entries, group):
    c = (entries + TASK_LANES[group] - 1) // TASK_LANES[group]
    return int(min(max(c, CHUNK_MIN), CHUNK_MAX))


def _part_ws_bytes(n, nbuckets, nwin):
    P = (nbuckets + PART_SUB - 1) // PART_SUB
    ntiles = (n + PART_TILE - 1) // PART_TILE
    maxblk = P + nwin * n // PART_CHUNK + 1
    return 1024 + nwin * n * 8 + 256 + 2 * (P * ntiles + 1) * 4 + (P + 1) * 4 + (P * ntiles // 2048 + 2) * 4 + 256 + maxblk * PART_SUB * 4


def plan(n, group, form):
    """dict(c, nwin, half, nbuckets, chunk, partition, graph, ws_bytes) of msm_plan (form 'resident') / msm_plan_direct (form 'oneshot')"""
    assert group in GROUPS and form in FORMS
    lg, xyw = _lg(n), 4 * COORD_WORDS[group]
    if form == "resident":
        c = 20 if lg >= 19 else 16 if lg >= 14 else 13 if lg >= 11 else 11 if lg == 10 else 10      # msm_plan
    else:
        c = min(max(lg - 3, 9), 16)                                                                  # msm_plan_direct
    nwin = (256 + 1 + c - 1) // c
    half = 1 << (c - 1)
    nbuckets = half if form == "resident" else nwin * half
    ent = nwin * n
    chunk = pick_chunk(ent, group)
    P = (nbuckets + PART_SUB - 1) // PART_SUB
    partition = n > 0 and ent >= PART_MIN_ENTRIES and P <= PART_MAXP
    b = 0
    if form == "resident":
        b += (nbuckets + 1) * 4 * 3
        b += 2 * ent * 4 + 256
        b += nbuckets * xyw * 4
        b += (2048 + 64 * 4) * xyw * 4
        b += (1024 + 3 * 1025) * 4 + 2 * (nbuckets + 1) * 4
        b += (nbuckets + ent // chunk + 2) * (8 + xyw * 4)
        b += 64 * 64 * xyw * 4 + 1024
        b += _part_ws_bytes(n, nbuckets, nwin)
        b += 4096
    else:
        b += (nbuckets + 1) * 4 * 3 + 2 * ent * 4 + 256 + nbuckets * xyw * 4
        b += nwin * (2048 + 64 * 4 + 1) * xyw * 4
        b += (1024 + 3 * 1025) * 4 + 2 * (nbuckets + 1) * 4
        b += (nbuckets + ent // chunk + 2) * (8 + xyw * 4)
        b += 64 * 64 * xyw * 4 + 1024
        b += _part_ws_bytes(n, nbuckets, nwin)
        b += 8192
    return dict(c=c, nwin=nwin, half=half, nbuckets=nbuckets, chunk=chunk, partition=bool(partition),
                graph=form == "resident" and n < GRAPH_MAX_N, ws_bytes=b)


def g1_resident_workspace_bytes(n):
    """zkt_g1_msm_workspace_bytes(n) (zkt_msm_handle.cpp): one slot's workspace plus `nwin * n * 97` bytes for the window-multiple table"""
    p = plan(n, "g1", "resident")
    return p["ws_bytes"] + p["nwin"] * n * 97


def window_bits(scalars, w, c):
    """bits [w*c, w*c + c) of every scalar of an (n, 4) uint64 array (k_digits' window_bits: bits at or above 256 read as zero)"""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    o = w * c
    word, sh = o >> 6, o & 63
    if word >= 4:
        return np.zeros(len(s), np.uint64)
    v = s[:, word] >> np.uint64(sh)
    if sh and word + 1 < 4:
        v |= s[:, word + 1] << np.uint64(64 - sh)
    return v & np.uint64((1 << c) - 1)


def digits(scalars, c, nwin):
    """k_digits restated: (mag, neg) as (nwin, n) arrays — signed c-bit digits with carry, raw > half is negative (magnitude 2^c - raw, carry 1)"""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    n, half = len(s), 1 << (c - 1)
    mag = np.zeros((nwin, n), np.int64)
    neg = np.zeros((nwin, n), bool)
    carry = np.zeros(n, np.int64)
    for w in range(nwin):
        raw = window_bits(s, w, c).astype(np.int64) + carry
        ng = raw > half
        mag[w] = np.where(ng, (1 << c) - raw, raw)
        neg[w] = ng
        carry = ng.astype(np.int64)
    return mag, neg


def bucket_ids(scalars, inf, c, nwin, form):
    """bucket of every (window, scalar) as an (nwin, n) array, -1 where k_digits writes no entry (magnitude 0, or an infinity base):
    mag - 1 (resident: one bucket set for all windows) or w * half + mag - 1 (one-shot: every window owns its buckets)"""
    mag, _ = digits(scalars, c, nwin)
    half = 1 << (c - 1)
    b = mag - 1
    if form == "oneshot":
        b = b + np.arange(nwin, dtype=np.int64)[:, None] * half
    live = mag != 0
    if inf is not None:
        live &= ~np.asarray(inf, bool)[None, :]
    return np.where(live, b, -1)


def census(scalars, inf, n, group, form):
    """per-bucket entry counts and the merge branch every bucket takes (k_task_count / k_task_scatter / k_merge_hot / k_merge_partials)"""
    p = plan(n, group, form)
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    assert len(s) == n
    b = bucket_ids(s, inf, p["c"], p["nwin"], form).ravel()
    count = np.bincount(b[b >= 0], minlength=p["nbuckets"]).astype(np.int64)
    ch = p["chunk"]
    nt = np.where(count <= ch, 1, (count + ch - 1) // ch)                 # ntasks_of: an empty bucket is one (empty) task too
    hot = int((nt > HOT_NT).sum())
    overflow = hot > HOT_CAP
    # k_merge_partials sums a many-piece bucket with coop_block_sum over its partials — or, if listed, over its HOT_FAN block sums (count 64: never bulk)
    block_counts = nt[(nt > MERGE_GROUP_MAX) & ((nt <= HOT_NT) | overflow)]
    return dict(plan=p, count=count, nt=nt,
                single=int((nt == 1).sum()),
                group=int(((nt >= 2) & (nt <= MERGE_GROUP_MAX)).sum()),
                block_lane_scatter=int(((nt > MERGE_GROUP_MAX) & (nt <= SCATTER_LANE_MAX)).sum()),
                block_scatter=int((nt > SCATTER_LANE_MAX).sum()),
                bulk=int((block_counts > BULK_MIN).sum()) if group != "g2" else 0,
                hot=hot, overflow=overflow, max_nt=int(nt.max()) if len(nt) else 0)


def scalars_from_ints(xs):
    """python ints (< 2^256) -> (n, 4) uint64"""
    out = np.zeros((len(xs), 4), np.uint64)
    for i, x in enumerate(xs):
        for j in range(4):
            out[i, j] = (x >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def ints_from_scalars(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


# ---- the GPU cases of tests/test_gpu_msm_plans.py -------------------------------------------------------------------------------
# Every case is a scalar vector plus the discrete logs k_i of its bases (base i = k_i * G), so the expected sum is (sum k_i s_i mod order) * G in
# python integers.  The sizes come from the plan, not from constants: a case states the branch it reaches, and test_msm_plan_model.py checks
# that claim against census() for every (group, form) before anything runs on a GPU.
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SECP_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
ORDER = {"g1": R_ORDER, "g2": R_ORDER, "secp": SECP_ORDER}
K_SAME = 0x2545F4914F6CDD1D5DEECE66D1234567                 # the one discrete log of the same-point cases
PLAN_N_MAX = 1 << 19
K_SEED = 20                                              # one random base set per group: every random-base case uses a prefix of it


class Case:
    def __init__(self, name, group, form, n, scalars, kspec, claim):
        self.name, self.group, self.form, self.n, self.scalars, self.kspec, self.claim = name, group, form, n, scalars, kspec, claim

    def ks(self):
        """(n, 4) uint64 discrete logs of the bases"""
        kind, arg = self.kspec
        if kind == "random":
            return random_ks(arg)[: self.n]
        k = np.tile(scalars_from_ints([arg]), (self.n, 1))
        if kind == "opposite":                                       # second half: -P = (order - k) G
            k[self.n // 2:] = scalars_from_ints([ORDER[self.group] - arg])[0]
        return k

    def census(self):
        return census(self.scalars, None, self.n, self.group, self.form)


_cache = {}


def random_ks(seed):
    """PLAN_N_MAX discrete logs < 2^254 (a prefix is the base set of a smaller case)"""
    key = ("k", seed)
    if key not in _cache:
        k = np.random.Generator(np.random.PCG64(seed)).integers(0, 2**64, size=(PLAN_N_MAX, 4), dtype=np.uint64)
        k[:, 3] >>= np.uint64(2)
        _cache[key] = k
    return _cache[key]


def random_scalars(seed, n, order):
    """n uniform scalars below `order` (a 320-bit draw reduced), as (n, 4) uint64"""
    key = ("s", seed, n, order)
    if key not in _cache:
        raw = np.random.Generator(np.random.PCG64(seed)).integers(0, 2**64, size=(n, 5), dtype=np.uint64)
        b = b"".join((int.from_bytes(r.tobytes(), "little") % order).to_bytes(32, "little") for r in raw)
        _cache[key] = np.frombuffer(b, dtype=np.uint64).reshape(n, 4).copy()
    return _cache[key]


def _random_avoiding(seed, count, p, form, avoid):
    """`count` uniform scalars none of whose entries falls into a bucket of `avoid` (so that the buckets a case fills hold exactly what it puts there)"""
    order = R_ORDER
    out, k = [], 0
    while sum(len(x) for x in out) < count:
        s = random_scalars(seed * 1000 + k, 2 * count + 64, order); k += 1
        b = bucket_ids(s, None, p["c"], p["nwin"], form)
        out.append(s[~np.isin(b, list(avoid)).any(axis=0)])
    return np.concatenate(out)[:count]


def _window_value(mags, c):
    """the scalar whose window w holds the positive digit mags[w] (every mags[w] < 2^(c-1): no carries)"""
    return sum(m << (c * w) for w, m in enumerate(mags))


def _bucket(p, form, w, mag):
    return mag - 1 + (w * p["half"] if form == "oneshot" else 0)


def case_hot_boundary(group, form, extra):
    """one bucket with exactly 512 * chunk + extra entries: nt = 512 (not hot) / 513 (hot, listed)"""
    n = 16384
    p = plan(n, group, form)
    target = HOT_NT * p["chunk"] + extra
    b0 = _bucket(p, form, 0, 1)
    s = np.concatenate([scalars_from_ints([1] * target), _random_avoiding(11, n - target, p, form, {b0})])
    return Case(f"hot-boundary-nt{HOT_NT + extra}", group, form, n, s, ("random", K_SEED),
                dict(max_nt=HOT_NT + extra, hot=extra, overflow=False, nt_of={b0: HOT_NT + extra}))


def _hot_values(p, count):
    """`count` scalars with 16 non-zero windows each, all (window, magnitude) pairs distinct and all magnitudes distinct: 16 * count buckets in both forms"""
    return [_window_value([16 * j + w + 1 for w in range(16)], p["c"]) for j in range(count)]


def case_hot_list(group, form, variant):
    """64 hot buckets (the listed k_merge_hot path at HOT_CAP), 65 (the list discarded), or ~10 random values repeated (well over HOT_CAP)"""
    n = 65536
    p = plan(n, group, form)
    thr = HOT_NT * p["chunk"] + 1                                      # entries that make a bucket hot
    if variant == "full64":
        vals = _hot_values(p, 4)
    elif variant == "over65":
        vals = _hot_values(p, 4) + [65]                              # one more bucket: magnitude 65 in window 0
    else:
        vals = ints_from_scalars(random_scalars(31, min(10, (n - 1024) // thr), R_ORDER))
    rep = scalars_from_ints([v for v in vals for _ in range(thr)])
    s = np.concatenate([rep, random_scalars(32, n - len(rep), R_ORDER)])
    claim = dict(hot=64, overflow=False) if variant == "full64" else dict(hot=65, overflow=True) if variant == "over65" else dict(hot_min=HOT_CAP + 1, overflow=True)
    return Case(f"hot-{variant}", group, form, n, s, ("random", K_SEED), claim)


MERGE_NTS = (8, 9, 16, 17, 64, 65)


def case_merge_thresholds(group, form):
    """buckets cut into exactly 8, 9, 16, 17, 64 and 65 pieces in one MSM: group vs block merge, lane vs block scatter, cooperative vs bulk sum"""
    n = 4096
    p = plan(n, group, form)
    mags = list(range(2, 2 + len(MERGE_NTS)))
    vals = [m for m, nt in zip(mags, MERGE_NTS) for _ in range(nt * p["chunk"])]
    want = {_bucket(p, form, 0, m): nt for m, nt in zip(mags, MERGE_NTS)}
    s = np.concatenate([scalars_from_ints(vals), _random_avoiding(41, n - len(vals), p, form, set(want))])
    claim = dict(nt_of=want, hot=0)
    if group != "g2":
        claim["bulk_min"] = 1
    return Case("merge-thresholds", group, form, n, s, ("random", K_SEED), claim)


def case_one_scalar(group, form, bases, regime):
    """every base the same point (bases 'same') or half P, half -P (bases 'opposite'), ONE scalar with one non-zero window: one bucket holds all n terms.
    regime 'bulk': 64 < nt <= 512 (k_merge_partials' one-lane sum, cooperative for G2); 'hot': nt > 512, listed (k_merge_hot)"""
    n = 2048 if regime == "bulk" else 8192
    p = plan(n, group, form)
    sc = 77
    s = scalars_from_ints([sc] * n)
    nt = n // p["chunk"]
    claim = dict(nt_of={_bucket(p, form, 0, sc): nt})
    if regime == "bulk":
        claim.update(hot=0)
        if group != "g2":
            claim["bulk"] = 1
    else:
        claim.update(hot=1, overflow=False)
    return Case(f"{bases}-point-{regime}", group, form, n, s, ("const" if bases == "same" else "opposite", K_SAME), claim)


def case_equal_bucket_sums(group, form):
    """every base the same point and every bucket of window 0 holding the same number of terms: all bucket sums equal (resident c = 16: scalars 1..half,
    one entry per bucket), so the marginals, the bit classes and the combine add equal points"""
    n = 32768
    p = plan(n, group, form)
    s = scalars_from_ints([(i % p["half"]) + 1 for i in range(n)])
    return Case("equal-bucket-sums", group, form, n, s, ("const", K_SAME), dict(equal_window0=n // p["half"]))


def case_infinity_result(group, form):
    """random bases and scalars, the last scalar chosen so that sum k_i s_i = 0 mod order: the result is the point at infinity"""
    n = 3000
    order = ORDER[group]
    s = random_scalars(51, n, order).copy()
    k = ints_from_scalars(random_ks(K_SEED)[:n])
    acc = sum(a * b for a, b in zip(k[:-1], ints_from_scalars(s[:-1]))) % order
    s[-1] = scalars_from_ints([(-acc * pow(k[-1], -1, order)) % order])[0]
    return Case("infinity-result", group, form, n, s, ("random", K_SEED), dict(total_zero=True))


def plan_steps(form):
    return RESIDENT_STEPS if form == "resident" else ONESHOT_STEPS


def case_plan_step(group, form, n):
    """uniform scalars with 0, 1, order - 1 and 2^256 - 1 mixed in, at one n of the step list"""
    order = ORDER[group]
    s = random_scalars(61, PLAN_N_MAX, order)[:n].copy()
    special = [0, 1, order - 1, (1 << 256) - 1]
    for i, v in zip((0, n // 3, n // 2, n - 1), special):
        s[i] = scalars_from_ints([v])[0]
    return Case(f"plan-n{n}", group, form, n, s, ("random", K_SEED), {})


def cases(group, form):
    """every case except the plan steps, as (id, builder) pairs; a builder returns the Case"""
    out = [(f"hot-boundary-{e}", lambda e=e: case_hot_boundary(group, form, e)) for e in (0, 1)]
    out += [(f"hot-{v}", lambda v=v: case_hot_list(group, form, v)) for v in ("full64", "over65", "many")]
    out += [("merge-thresholds", lambda: case_merge_thresholds(group, form))]
    out += [(f"{b}-{r}", lambda b=b, r=r: case_one_scalar(group, form, b, r)) for b in ("same", "opposite") for r in ("bulk", "hot")]
    out += [("equal-bucket-sums", lambda: case_equal_bucket_sums(group, form))]
    out += [("infinity-result", lambda: case_infinity_result(group, form))]
    return out


def check_claim(case):
    """[] if census(case) shows every branch the case claims, else the list of what differs"""
    cen, bad = case.census(), []
    for key, want in case.claim.items():
        if key in ("hot", "overflow", "max_nt", "bulk") and cen[key] != want:
            bad.append(f"{key} = {cen[key]}, claimed {want}")
        elif key == "hot_min" and cen["hot"] < want:
            bad.append(f"hot = {cen['hot']}, claimed at least {want}")
        elif key == "bulk_min" and cen["bulk"] < want:
            bad.append(f"bulk = {cen['bulk']}, claimed at least {want}")
        elif key == "nt_of":
            for b, nt in want.items():
                if cen["nt"][b] != nt:
                    bad.append(f"bucket {b}: nt = {cen['nt'][b]}, claimed {nt}")
        elif key == "equal_window0":
            cnt = cen["count"][: cen["plan"]["half"]]
            if not (cnt == want).all():
                bad.append(f"window-0 bucket counts {sorted(set(cnt.tolist()))[:5]}, claimed all {want}")
        elif key == "total_zero":
            order = ORDER[case.group]
            if sum(a * b for a, b in zip(ints_from_scalars(case.ks()), ints_from_scalars(case.scalars))) % order:
                bad.append("sum k_i s_i is not 0 mod order")
    return bad
