"""The layout of a host-pointer call's staging slots (csrc/host_stage.h: stage_layout, from which Stage::commit both reserves and carves the arena) in the host
build of the library's host code (libzkt_hostcheck.so).  No GPU.

Every list of sizes from SIZES at every slot count up to the capacity: zero-byte slots, sizes one either side of the 256-byte alignment, and one past 2^20."""
import ctypes, itertools, os
import pytest
from zkt_testlib import ROOT

SIZES = (0, 1, 255, 256, 257, 4095, 2**20 + 1)
pad = lambda b: (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "zk-toolkit_amd", "libzkt_hostcheck.so")
    assert os.path.exists(so), "build first (__graft_entry__.build())"
    h = ctypes.CDLL(so)
    h.zkt_hostcheck_stage_layout.restype = ctypes.c_size_t
    return h


def test_capacity_holds_the_widest_call(H):
    assert H.zkt_hostcheck_stage_slots() == 6          # ECDSA signing from messages: messages, offsets, keys, nonces, signatures, flags


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 6])
def test_offsets_aligned_ordered_disjoint_and_total_exact(H, count):
    assert count <= H.zkt_hostcheck_stage_slots()
    arr = ctypes.c_size_t * count
    off = arr()
    for sizes in itertools.product(SIZES, repeat=count):
        off[:] = [2**64 - 1] * count
        total = H.zkt_hostcheck_stage_layout(arr(*sizes), count, off)
        o = list(off)
        assert all(x % 256 == 0 for x in o), (sizes, o)
        assert o[0] == 0 and all(o[i + 1] >= o[i] + sizes[i] for i in range(count - 1)), (sizes, o)
        assert total >= o[-1] + sizes[-1], (sizes, o, total)
        assert total == sum(pad(b) for b in sizes), (sizes, total)
