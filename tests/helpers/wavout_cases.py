"""Inputs the host and the device tests of the wav back end share (tests/test_wavout_host.py, tests/test_gpu_wavout.py)."""
import numpy as np


def special_values(width):
    """(samples, integers, clipped) for an integer target of ``width`` bytes: +-0.5, 1.5 and 2.5 LSB (halves go to even), +-1.0,
    +-1.5, NaN, +-inf and 0.  Every input is an exact fp32 value."""
    bits = 8 * width - 1
    lsb, top = 2.0 ** -bits, 2 ** bits
    x = [0.5 * lsb, -0.5 * lsb, 1.5 * lsb, -1.5 * lsb, 2.5 * lsb, -2.5 * lsb, 1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.0]
    v = [0, 0, 2, -2, 2, -2, top - 1, -top, top - 1, -top, 0, top - 1, -top, 0]
    x32 = np.array(x, dtype=np.float32)
    assert np.array_equal(x32.astype(np.float64), np.array(x), equal_nan=True)
    return x32, v, 6                                      # clipped: +1.0, +-1.5, NaN, +-inf
