"""Which entry points of include/zkt.h promise stream ordering, and what tests/test_gpu_stream_order.py relies on to test it.

TEST INFRASTRUCTURE.  INTEGRATION.md promises that "entry points that take a `stream` argument order their work behind it".  This file
  - reads include/zkt.h for every prototype with a `void* stream` parameter (stream_functions),
  - maps each of them to the delayed-producer case of tests/test_gpu_stream_order.py that tests the promise, or to the reason it needs none (TABLE),
  - restates the constants of zk-toolkit_amd/csrc/zkt_msm_handle.cpp that the pipeline cases are built on, each with the source line it restates
    (SOURCE_LINES), so that whoever changes the slot count, the graph cache, the reduce streams or the large-set threshold is sent to the GPU cases.
tests/test_stream_order_model.py checks all three on the CPU."""
import ast, os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkt.h")
HANDLE_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_msm_handle.cpp")
COMM_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_comm.cpp")
API_SRC = os.path.join(ROOT, "zk-toolkit_amd", "csrc", "zkt_api.cpp")
GPU_MODULE = os.path.join(ROOT, "tests", "test_gpu_stream_order.py")

GROUPS = ("g1", "g2", "secp")

# ---- constants of zkt_msm_handle.cpp the GPU cases are built on ----------------------------------------------------------------------
MSM_SLOTS = 8               # `constexpr int MSM_SLOTS = 8;` (and ZKT_MSM_SLOTS of the header): the small-path case keeps all of them in flight
NGRAPH = 4                  # MsmSlot `static constexpr int NGRAPH = 4;`: graphs cached per slot, keyed by the scalar vector's address
NTAIL = 8                   # zkt_bases_impl `static constexpr int NTAIL = 8;`: a small set runs slot k on reduce stream k % NTAIL
LARGE_LOG2 = 19             # `const bool small = h.n < (size_t(1) << 19);`: from 2^19 terms on, sort | accumulate | reduce run on three streams
LARGE_TAILS = 2             # slot_tail_stream `... : slot % 2].s;`: a large set uses two reduce streams, so slots of equal parity share one
BATCH_MAX_LOG2 = 19         # msm_batch_submit `n >= (size_t(1) << 19)` is ZKT_ERR_SHAPE: the batch exists on the small path only

# the lines restated above and the waits the delayed-producer cases exist for: (what, file, text that must occur, how often)
SOURCE_LINES = [
    ("MSM_SLOTS", HANDLE_SRC, "constexpr int MSM_SLOTS = %d;" % MSM_SLOTS, 1),
    ("ZKT_MSM_SLOTS", HEADER, "#define ZKT_MSM_SLOTS %d" % MSM_SLOTS, 1),
    ("NGRAPH", HANDLE_SRC, "static constexpr int NGRAPH = %d;" % NGRAPH, 1),
    ("NTAIL", HANDLE_SRC, "static constexpr int NTAIL = %d;" % NTAIL, 1),
    ("large-set threshold", HANDLE_SRC, "const bool small = h.n < (size_t(1) << %d);" % LARGE_LOG2, 2),        # slot_tail_stream and msm_submit
    ("reduce stream of a slot", HANDLE_SRC, "return h.s_tail[small ? slot %% zkt_bases_impl::NTAIL : slot %% %d].s;" % LARGE_TAILS, 1),
    ("sort stream of a large set", HANDLE_SRC, "hipStream_t ss = small ? st : h.s_sort.s;", 1),
    ("batch stream", HANDLE_SRC, "hipStream_t batch_stream(const zkt_bases_impl& h) { return slot_tail_stream(h, MSM_SLOTS - 1); }", 1),
    ("batch size limit", HANDLE_SRC, "n >= (size_t(1) << %d)" % BATCH_MAX_LOG2, 1),
    ("input event of a slot", HANDLE_SRC, "HIPCHK(hipEventRecord(F.e_in.e, (hipStream_t)stream));", 2),      # msm_submit and msm_batch_submit
    ("input wait of msm_submit", HANDLE_SRC, "HIPCHK(hipStreamWaitEvent(ss, F.e_in.e, 0));", 1),
    ("input wait of msm_batch_submit", HANDLE_SRC, "HIPCHK(hipStreamWaitEvent(st, F.e_in.e, 0));", 1),
    ("msm_dev is submit + collect on slot 0", HANDLE_SRC, "ZCHK(msm_submit(h, k, n, stream, 0)); return msm_collect(h, 0, out, partial); }); }", 1),
    ("input wait of zkt_tate_batch_dev", API_SRC, "HIPCHK(hipStreamWaitEvent(s, g_tate_ev[0], 0));", 1),
    # zkt_comm.cpp:220-224: zkt_*_msm_sharded hands its stream to zkt_*_msm_dev unchanged
    ("msm_sharded passes its stream on", COMM_SRC, "int rc = out ? zkt_##NAME##_msm_dev(b, dev_scalars, n_local, stream, nullptr, send_payload()) : ZKT_ERR_SHAPE;", 1),
]


def large(n):
    """does a resident set of n terms take the three-stream branch of msm_submit"""
    return n >= 1 << LARGE_LOG2


def tail_stream_index(n, slot):
    """index of the reduce stream slot_tail_stream gives a slot of an ungrouped handle"""
    return slot % LARGE_TAILS if large(n) else slot % NTAIL


def source_line_counts():
    """[(what, wanted count, found count)] for SOURCE_LINES"""
    text, out = {}, []
    for what, path, line, count in SOURCE_LINES:
        if path not in text:
            with open(path) as f:
                text[path] = f.read()
        out.append((what, count, text[path].count(line)))
    return out


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def stream_functions(header=HEADER):
    """every function of the header with a `void* stream` parameter, in the header's order"""
    with open(header) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = []
    for m in re.finditer(r"\b(zkt_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", txt, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)) and m.group(1) not in out:
            out.append(m.group(1))
    return out


# ---- symbol -> ("case", id of a case of tests/test_gpu_stream_order.py) | ("exempt", reason) -----------------------------------------
SHARDED_EXEMPT = ("zkt_comm.cpp:220-224: the call holds the communicator's lock and hands `stream` unchanged to zkt_%s_msm_dev, whose case covers the ordering; "
                  "the rest is the exchange and the combine, which need a communicator: tests/test_gpu_combine.py (world 1, and the combine kernel on a caller "
                  "stream) and tests/comm_cases_worker.py (worlds 3 and 8) run them against python integers")
TABLE = {
    "zkt_fq_mul_batch_dev": ("case", "fq_mul_batch_dev"),
    "zkt_g1_mul_batch_dev": ("case", "g1_mul_batch_dev"),
    "zkt_g2_mul_batch_dev": ("case", "g2_mul_batch_dev"),
    "zkt_tate_batch_dev": ("case", "tate_batch_dev"),
    "zkt_fr_poly_mul_dev": ("case", "fr_poly_mul_dev"),
    "zkt_ecdsa_verify_digest_batch_dev": ("case", "ecdsa_verify_digest_batch_dev"),
    "zkt_ed25519_verify_batch_dev": ("case", "ed25519_verify_batch_dev"),
}
for _g in GROUPS:
    for _f in ("bases_from_device", "jac_sum_dev", "msm_dev", "msm_submit", "msm_batch_submit", "msm_batch_dev"):
        TABLE[f"zkt_{_g}_{_f}"] = ("case", f"{_g}_{_f}")
    TABLE[f"zkt_{_g}_msm_sharded"] = ("exempt", SHARDED_EXEMPT % _g)


def case_ids():
    """ids of the delayed-producer cases the table names, in the table's order"""
    return [v for k, v in TABLE.values() if k == "case"]


def defined_cases(module=GPU_MODULE):
    """ids the GPU module defines with its @case("id") decorator, read from its source (no import: it needs torch and a device)"""
    with open(module) as f:
        tree = ast.parse(f.read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef):
            for d in node.decorator_list:
                if isinstance(d, ast.Call) and getattr(d.func, "id", None) == "case":
                    out += [a.value for a in d.args if isinstance(a, ast.Constant)]
    return out


def table_problems(header=HEADER, module=GPU_MODULE):
    """[] when every `void* stream` function of the header has a table entry, every entry is a function of the header, and every case named exists once"""
    fns, bad = stream_functions(header), []
    bad += [f"{f}: takes a stream and has no entry in stream_order_model.TABLE" for f in fns if f not in TABLE]
    bad += [f"{f}: in TABLE but not a `void* stream` function of the header" for f in TABLE if f not in fns]
    have = defined_cases(module)
    for f, (kind, what) in TABLE.items():
        if kind == "case" and have.count(what) != 1:
            bad.append(f"{f}: case {what!r} is defined {have.count(what)} times in {os.path.basename(module)}")
        if kind == "exempt" and not what.strip():
            bad.append(f"{f}: exempt without a reason")
    ids = case_ids()
    bad += [f"case {c!r} of {os.path.basename(module)} is named by no table entry" for c in have if c not in ids]
    bad += [f"case {c!r} is named by more than one table entry" for c in set(ids) if ids.count(c) > 1]
    return bad
