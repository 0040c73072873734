"""The float64 definition of the rational polyphase converter for an arbitrary pair of rates, an arbitrary n_out and either input layout
-- the restatement of tests/test_gpu_resample.py (which fixes sr_out = 44100 and n_out = ceil(n_in L / M)) generalised for the writer-side
form, asx_resample_rational_stem:

    y[m] = sum_i x[i] h[m M - i L],  0 <= i < n_in,  |m M - i L| <= half,   for every 0 <= m < n_out the caller asks for

so an output past ceil(n_in L / M) is the same sum, and exactly 0 from ``zero_from`` on, where the filter has left the input.  Helper
module of tests/test_host_output_rate.py and tests/test_gpu_resample_stem.py; no test of its own."""
import math

import numpy as np

_DESIGN = {}


def design(sr_in, sr_out):
    """(L, M, half, T, taps float64 [2 half + 1]) of sr_in -> sr_out Hz (the design of csrc/resample_plan.h, restated with scipy /
    numpy); computed once per pair."""
    key = (int(sr_in), int(sr_out))
    if key not in _DESIGN:
        from scipy.signal import kaiserord
        g = math.gcd(*key)
        L, M = key[1] // g, key[0] // g
        G = max(L, M)
        fpass, fstop = 0.913 / G, 1.0 / G
        N, beta = kaiserord(125.0, fstop - fpass)
        half = -(-(N - 1) // (2 * L)) * L
        n = np.arange(-half, half + 1, dtype=np.float64)
        fc = 0.5 * (fpass + fstop)
        h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
        h *= L / h.sum()
        h.flags.writeable = False
        _DESIGN[key] = (L, M, half, 2 * half // L + 1, h)
    return _DESIGN[key]


def tile(L, M, T):
    """(J, K, span, floats of LDS) of the workgroup tile -- the rule of csrc/resample_plan.h: K = 8 periods (halved while one period does
    not fit), J the multiple of L up to 1024 that fills the 256-thread passes best (the largest on ties), inside 16384 floats of LDS
    together with a table of at most 2048 floats."""
    taps = L * T if L * T <= 2048 else 0
    budget = 16384 - taps
    K = 8
    while K > 1 and K * M + T > budget:
        K //= 2
    assert K * M + T <= budget
    best, J, kg = -1.0, L, 1
    while kg * L <= max(L, 1024) and kg * K * M + T <= budget:
        eff = kg * L / (-(-kg * L // 256) * 256)
        if eff >= best:
            best, J = eff, kg * L
        kg += 1
    span = J // L * K * M + T
    return J, K, span, span + taps


def tile_outputs(L, M, T):
    """Consecutive outputs one workgroup owns."""
    J, K, _, _ = tile(L, M, T)
    return J * K


def plan_n_out(n_in, L, M):
    return -(-n_in * L // M)


def zero_from(n_in, L, M, half):
    """The first output index from which every y[m] is exactly 0: m M - (n_in - 1) L > half."""
    return ((n_in - 1) * L + half) // M + 1


def reference(x, sr_in, sr_out, n_out=None, layout="planar"):
    """float64 planar [C, n_out] by the definition; x planar [C, n_in] (or [n_in]) or rows [n_in, C].  For tap row t the input index is
    q + P - t and the tap index (m M mod L) + (t - P) L."""
    L, M, half, T, h = design(sr_in, sr_out)
    xd = np.asarray(x, np.float64)
    if layout == "rows":
        xd = xd.T
    n_in = xd.shape[-1]
    if n_out is None:
        n_out = plan_n_out(n_in, L, M)
    m = np.arange(n_out, dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    P = half // L
    y = np.zeros(xd.shape[:-1] + (n_out,), np.float64)
    for t in range(T):
        i = q + P - t
        n = p + (t - P) * L
        ok = (i >= 0) & (i < n_in) & (np.abs(n) <= half)
        if ok.any():
            y[..., ok] += xd[..., i[ok]] * h[n[ok] + half]
    return y


def output_frames(n, file_frames, file_rate, model_rate):
    """The length rule of asx_output_rate = "input": a stem of n samples at the model's rate -> frames at the file's rate."""
    return min(file_frames, -(-n * file_rate // model_rate))
