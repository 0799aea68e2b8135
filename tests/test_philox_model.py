"""The host model of the kernels' Philox4x32-7 (tests/helpers.py, csrc/pbhc_math.h philox4x32): the general four-word form against the
published known-answer vectors of Random123 (philox4x32_7), and the observation-noise wrapper `_philox4x32_7_word0` against the values it
returned before it became a wrapper."""
import numpy as np

from tests import helpers


def test_philox4x32_7_known_answers():
    M = 0xFFFFFFFF
    kat = [((0, 0, 0, 0), 0, (0x5f6fb709, 0x0d893f64, 0x4f121f81, 0x4f730a48)),
           ((M, M, M, M), (M << 32) | M, (0x5207ddc2, 0x45165e59, 0x4d8ee751, 0x8c52f662)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0x299f31d0 << 32) | 0xa4093822, (0x4dfccaba, 0x190a87f0, 0xc47362ba, 0xb6b5242a))]
    for ctr, key, want in kat:
        got = helpers._philox4x32_7(key, *ctr)
        assert tuple(int(w) for w in got) == want


def test_word0_wrapper_is_unchanged():
    pinned = [(0, np.arange(4), 0, [0x93ff5018, 0x248cce1b, 0x903aadbe, 0x3d9a94f1]),
              (1234, np.array([0, 1, 7, 4095]), 7, [0x753d51b6, 0x77545454, 0xdbd07efb, 0x7ff6a9bd]),
              (0x9E3779B97F4A7C15, np.array([3, 2 ** 31 + 5, 2 ** 32 - 1]), 2 ** 24 + 3, [0xb88524fa, 0x244201f0, 0xaa9b71b5])]
    for seed, ids, ctr, want in pinned:
        got = helpers._philox4x32_7_word0(seed, ids.astype(np.int64), ctr)
        assert got.dtype == np.uint64 and got.shape == ids.shape and [int(x) for x in got] == want
        full = helpers._philox4x32_7(seed, ids, ctr, 16, 0)
        assert len(full) == 4 and np.array_equal(full[0], got)


def test_words_broadcast_and_depend_on_every_counter_word():
    rows, lanes = np.arange(5)[:, None], np.arange(3)[None, :]
    o = helpers._philox4x32_7(77, rows, 9, 0x5A4D, lanes)
    assert all(w.shape == (5, 3) for w in o)
    assert not np.array_equal(o[0], helpers._philox4x32_7(77, 9, rows, 0x5A4D, lanes)[0])          # c0 and c1 are not interchangeable
    assert len(np.unique(o[0])) == 15 and len(np.unique(o[1])) == 15
