"""The float32 restatement of the file-rate complement (asx_resample_rational_complement, ``asx_complement_rate`` = "input"):

    c = fl( fl(s * mix) - fl(k * y) )

with numpy float32 arrays, so every operation rounds once to float32 and nothing is fused.  Helper module of
tests/test_gpu_resample_complement.py, tests/test_gpu_complement_rate.py and tests/test_host_complement_rate.py (which holds it against a
float64 evaluation); no test of its own."""
import numpy as np

# three float32 roundings on magnitudes <= 1.65 (k y), 1 (s mix) and 2.65 (the difference), each within 2^-24 relative: for inputs in
# [-1, 1], s <= 1, k <= 1.1 and |y| <= 1.5 the restatement lies within 6 * 2^-24 of the exact s mix - k y
ROUNDING_BOUND = 6.0 * 2.0 ** -24


def complement_f32(mix, y, s, k):
    """mix, y: float32 arrays of one shape; s, k: the scales (rounded to float32 first, as the C entry receives them)."""
    mix, y = np.asarray(mix), np.asarray(y)
    assert mix.dtype == np.float32 and y.dtype == np.float32 and mix.shape == y.shape
    a = np.float32(s) * mix
    b = np.float32(k) * y
    c = a - b
    assert a.dtype == b.dtype == c.dtype == np.float32
    return c


def complement_f64(mix, y, s, k):
    """The same value without rounding (float64 on the float32 scales)."""
    return float(np.float32(s)) * np.asarray(mix, np.float64) - float(np.float32(k)) * np.asarray(y, np.float64)
