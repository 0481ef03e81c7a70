"""bench.py --dump-outputs writes the point the timed MSM returns as float64 words.  The format is checked here without a GPU: every
word must come back exactly, so two builds can be compared output for output."""
import numpy as np

import bench
from zkt_testlib import G1_GEN, g1_arr


def _read_back(words):
    w = [int(v) for v in words]
    x = sum(v << (32 * i) for i, v in enumerate(w[:12]))
    y = sum(v << (32 * i) for i, v in enumerate(w[12:24]))
    return x, y, w[24]


def test_dump_outputs_is_exact(tmp_path):
    pt = g1_arr([G1_GEN])
    pt[0, 12] |= np.uint64(0xA5A5A5A5) << np.uint64(32)          # the padding word of zkt_g1_affine is not part of the output
    bench.dump_outputs(str(tmp_path / "out"), pt)
    a = np.load(tmp_path / "out" / "g1_msm_last_step.npy")
    assert a.dtype == np.float64 and a.shape == (25,)
    assert (a == np.floor(a)).all() and (a >= 0).all() and (a < 2**32).all()
    assert _read_back(a) == (G1_GEN[0], G1_GEN[1], 0)


def test_dump_outputs_point_at_infinity(tmp_path):
    bench.dump_outputs(str(tmp_path), g1_arr([None]))
    assert _read_back(np.load(tmp_path / "g1_msm_last_step.npy")) == (0, 0, 1)
