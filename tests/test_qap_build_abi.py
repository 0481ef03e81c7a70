"""Shape errors of the R1CS -> QAP entry points (zkt_qap_build, zkt_qap_create) and of the _resident calls: ZKT_ERR_SHAPE with every output untouched.  The
arguments are checked before the device is asked for, so these run the same with and without a GPU."""
import ctypes, importlib
import numpy as np
import pytest
from zkt_testlib import ptr, ZKT_ERR_SHAPE, G1W, G2W
from qap_util import sparse_struct, alloc_crs

zk = importlib.import_module("zk-toolkit_amd")
PAT = 0xABABABABABABABAB
MAX_N, MAX_CELLS = 8192, 1 << 26


def _mat(n, entries=()):
    """CSR of n rows from (row, col, value) entries given in row order"""
    rowptr = np.zeros(n + 1, np.uint64); col = []; val = []
    for j, i, v in entries:
        rowptr[j + 1:] += np.uint64(1); col.append(i); val.append([v, 0, 0, 0])
    return rowptr, np.array(col if col else [0], np.uint32), np.array(val if val else [[0, 0, 0, 0]], np.uint64)


def _outs(cells=8):
    return [np.full((cells, 4), PAT, np.uint64) for _ in range(3)]


def _untouched(*arrays):
    return all((a == np.uint64(PAT)).all() for a in arrays)


def _both(n, cols, structs, expect_index=None):
    """zkt_qap_build and zkt_qap_create on the same arguments: ZKT_ERR_SHAPE, outputs and the handle slot untouched"""
    L = zk.lib()
    refs = [ctypes.byref(s) if s is not None else None for s in structs]
    outs = _outs()
    assert L.zkt_qap_build(n, cols, *refs, *(ptr(o) for o in outs)) == ZKT_ERR_SHAPE
    if expect_index is not None: assert L.zkt_last_error_index() == expect_index
    assert _untouched(*outs)
    h = ctypes.c_void_p(0xABAB)
    assert L.zkt_qap_create(n, cols, *refs, ctypes.byref(h)) == ZKT_ERR_SHAPE
    if expect_index is not None: assert L.zkt_last_error_index() == expect_index
    assert h.value == 0xABAB


GOOD = [(0, 0, 1), (1, 1, 2), (1, 2, 3), (3, 0, 4)]        # 4 rows over 3 columns


def _good(): return [sparse_struct(*_mat(4, GOOD)) for _ in range(3)]


def test_null_pointers_and_zero_sizes():
    L = zk.lib()
    for k in range(3):
        s = _good(); s[k] = None
        _both(4, 3, s)
    for k in range(3):                                        # a null rowptr inside a matrix
        s = _good(); whole = s[k]; s[k] = type(whole)(None, whole.col, whole.val)
        _both(4, 3, s)
    _both(0, 3, _good()); _both(4, 0, _good())
    s = _good(); refs = [ctypes.byref(x) for x in s]
    for k in range(3):                                        # a null output of zkt_qap_build: the other two stay untouched
        outs = _outs(12); ps = [ptr(o) for o in outs]; ps[k] = None
        assert L.zkt_qap_build(4, 3, *refs, *ps) == ZKT_ERR_SHAPE and _untouched(*outs)
    assert L.zkt_qap_create(4, 3, *refs, None) == ZKT_ERR_SHAPE


def test_limits():
    one_row = lambda n: [sparse_struct(*_mat(n)) for _ in range(3)]
    _both(MAX_N + 1, 1, one_row(MAX_N + 1))                  # n = 8193
    assert 265 * 253241 == MAX_CELLS + 1
    _both(265, 253241, one_row(265))                         # cols * n = 2^26 + 1
    _both(1, MAX_CELLS + 1, one_row(1))
    _both(MAX_N, MAX_CELLS // MAX_N + 1, one_row(MAX_N))
    _both(2, 1 << 63, one_row(2))                            # cols * n wraps to 0


def test_bad_rowptr():
    for k in range(3):
        s = _good(); rp, col, val = _mat(4, GOOD); rp[0] = 1
        s[k] = sparse_struct(rp, col, val); _both(4, 3, s)                                   # rowptr[0] != 0
        s = _good(); rp, col, val = _mat(4, GOOD); rp[2] = 0
        s[k] = sparse_struct(rp, col, val); _both(4, 3, s, expect_index=1)                   # row 1 ends before it starts
        s = _good(); rp, col, val = _mat(4, GOOD); rp[4] = 0xFFFFFFFF
        s[k] = sparse_struct(rp, col, val); _both(4, 3, s)                                   # too many entries (nothing past the four stored ones is read)


def test_column_out_of_range_reports_its_row():
    for k in range(3):
        s = _good(); rp, col, val = _mat(4, GOOD); col[2] = 3                                # col == cols, in row 1
        s[k] = sparse_struct(rp, col, val); _both(4, 3, s, expect_index=1)
        s = _good(); rp, col, val = _mat(4, GOOD); col[3] = 0xFFFFFFFF                       # in row 3
        s[k] = sparse_struct(rp, col, val); _both(4, 3, s, expect_index=3)
    s = _good(); rp, col, val = _mat(4, GOOD); col[0] = 7                                    # A's row 3 and B's row 0: A is looked at first
    rp2, col2, val2 = _mat(4, GOOD); col2[3] = 7
    s[0] = sparse_struct(rp2, col2, val2); s[1] = sparse_struct(rp, col, val); _both(4, 3, s, expect_index=3)


def test_resident_calls_reject_null_arguments_with_outputs_untouched():
    L = zk.lib()
    w = np.ones((3, 4), np.uint64); h = np.full((4, 4), PAT, np.uint64)
    assert L.zkt_qap_quotient_resident(None, ptr(w), ptr(h)) == ZKT_ERR_SHAPE and _untouched(h)
    assert L.zkt_qap_download(None, ptr(h), ptr(h), ptr(h)) == ZKT_ERR_SHAPE and _untouched(h)
    L.zkt_qap_free(None)                                                                     # a no-op
    crs, bufs = alloc_crs(4, 1, 2)
    for b in bufs.values(): b[:] = np.uint64(PAT)
    k = np.ones((1, 4), np.uint64)
    assert L.zkt_groth16_setup_resident(ctypes.byref(crs), None, ptr(k), ptr(k), ptr(k), ptr(k), ptr(k)) == ZKT_ERR_SHAPE
    assert L.zkt_groth16_setup_resident(None, None, ptr(k), ptr(k), ptr(k), ptr(k), ptr(k)) == ZKT_ERR_SHAPE
    assert _untouched(*bufs.values())
    A = np.full((1, G1W), PAT, np.uint64); B = np.full((1, G2W), PAT, np.uint64); C = np.full((1, G1W), PAT, np.uint64)
    assert L.zkt_groth16_prove_resident(ctypes.byref(crs), None, ptr(w), ptr(k), ptr(k), ptr(A), ptr(B), ptr(C)) == ZKT_ERR_SHAPE
    assert L.zkt_groth16_prove_resident(None, None, ptr(w), ptr(k), ptr(k), ptr(A), ptr(B), ptr(C)) == ZKT_ERR_SHAPE
    assert _untouched(A, B, C)
