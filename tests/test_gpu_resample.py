"""asx_resample_rational -- the rational polyphase converter that brings an input file to the model's sample rate on the device --
against the float64 evaluation of its definition, restated here in numpy (the design as in tests/test_host_resample_plan.py):

    y[m] = sum_i x[i] h[m M - i L],  0 <= i < n_in,  |m M - i L| <= half;   n_out = ceil(n_in L / M)

Bound: 1e-6 max abs on inputs in [-1, 1].  A float32 dot product with float32 taps differs from float64 by <= 2.5e-7 on unit sines; the
bound leaves 4x for the kernel's summation order (two chains from the ends of the filter towards its centre)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-6
PAIRS = [(48000, 147, 160), (96000, 147, 320), (22050, 2, 1), (32000, 441, 320), (88200, 1, 2), (8000, 441, 80), (192000, 147, 640)]
SR_OUT = 44100


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


_DESIGN = {}


def design(sr_in):
    """(L, M, half, T, taps float64 [2 half + 1]) of sr_in -> 44100 Hz; computed once per rate."""
    if sr_in not in _DESIGN:
        from scipy.signal import kaiserord
        g = math.gcd(sr_in, SR_OUT)
        L, M = SR_OUT // g, sr_in // g
        G = max(L, M)
        fpass, fstop = 0.913 / G, 1.0 / G
        N, beta = kaiserord(125.0, fstop - fpass)
        half = -(-(N - 1) // (2 * L)) * L
        n = np.arange(-half, half + 1, dtype=np.float64)
        fc = 0.5 * (fpass + fstop)
        h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
        h *= L / h.sum()
        h.flags.writeable = False
        _DESIGN[sr_in] = (L, M, half, 2 * half // L + 1, h)
    return _DESIGN[sr_in]


def tile_outputs(L, M, T):
    """Consecutive outputs one workgroup owns (the rule of csrc/resample_plan.h: J a multiple of L up to 1024 that fills the 256-thread
    passes best, K = 8 periods, inside 16384 floats of LDS)."""
    lds = L * T if L * T <= 2048 else 0
    K = 8
    best, J = -1.0, L
    kg = 1
    while kg * L <= max(L, 1024) and kg * K * M + T <= 16384 - lds:
        eff = kg * L / (-(-kg * L // 256) * 256)
        if eff >= best:
            best, J = eff, kg * L
        kg += 1
    return J * K


def reference(x, sr_in):
    """float64, by the definition: for tap row t the input index is q + P - t and the tap index (m M mod L) + (t - P) L."""
    L, M, half, T, h = design(sr_in)
    n_in = x.shape[-1]
    n_out = -(-n_in * L // M)
    m = np.arange(n_out, dtype=np.int64)
    q, p = (m * M) // L, (m * M) % L
    P = half // L
    y = np.zeros(x.shape[:-1] + (n_out,), np.float64)
    xd = x.astype(np.float64)
    for t in range(T):
        i = q + P - t
        n = p + (t - P) * L
        ok = (i >= 0) & (i < n_in) & (np.abs(n) <= half)
        if ok.any():
            y[..., ok] += xd[..., i[ok]] * h[n[ok] + half]
    return y


def lengths(sr_in):
    L, M, _, T, _ = design(sr_in)
    tile = tile_outputs(L, M, T)
    edge = -(-tile * M // L)              # the shortest input with a whole tile of outputs
    return sorted({1, 2, T - 1, 4000, 256 * 14 + 1, edge - 1, edge, edge + 1, edge + 2})


def signals(sr_in, n, channels):
    rng = np.random.default_rng(n * 7 + channels)
    noise = rng.uniform(-1.0, 1.0, (channels, n)).astype(np.float32)
    i = np.arange(n, dtype=np.float64)
    f = np.array([0.31, 0.83])[:channels, None] * min(sr_in, SR_OUT) / 2.0
    sine = np.sin(2.0 * np.pi * f * i / sr_in + np.array([0.4, 2.1])[:channels, None]).astype(np.float32)
    return {"noise": noise, "sine": sine}


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("sr_in,L,M", PAIRS)
def test_against_float64_definition(eng, sr_in, L, M, channels):
    dL, dM, _, T, _ = design(sr_in)
    assert (dL, dM) == (L, M)
    worst = 0.0
    for n in lengths(sr_in):
        n_out, pL, pM, pT = eng.resample_rational_plan(sr_in, SR_OUT, n)
        assert (n_out, pL, pM, pT) == (-(-n * L // M), L, M, T)
        for name, x in signals(sr_in, n, channels).items():
            got = eng.resample_rational(x, sr_in, SR_OUT)
            assert got.shape == (channels, n_out) and got.dtype == np.float32
            ref = reference(x, sr_in)
            err = np.abs(got - ref)
            worst = max(worst, float(err.max()))
            assert err.max() <= TOL, (sr_in, n, name, float(err.max()), int(err.argmax()))
            # the zero-history edges
            assert err[:, :T].max() <= TOL and err[:, -T:].max() <= TOL
    print(f"{sr_in} -> {SR_OUT}, {channels} ch: max |kernel - float64| = {worst:.3e}")


def test_mono_vector_and_refusals(eng):
    import audio_separator_amd as A
    x = signals(48000, 1000, 1)["noise"]
    y = eng.resample_rational(x[0], 48000, SR_OUT)
    assert y.shape == (919,)
    np.testing.assert_array_equal(y, eng.resample_rational(x, 48000, SR_OUT)[0])
    with pytest.raises(A.AsxError, match="equal"):
        eng.resample_rational(x, SR_OUT, SR_OUT)
    with pytest.raises(A.AsxError, match="2\\^20"):
        eng.resample_rational(x, 44056, SR_OUT)


@pytest.mark.parametrize("sr_in", [48000, 22050])
def test_runs_are_bit_identical_and_dev_equals_host(eng, sr_in):
    import torch
    L, M, _, T, _ = design(sr_in)
    n = -(-tile_outputs(L, M, T) * M // L) + 777
    x = signals(sr_in, n, 2)["noise"]
    a = eng.resample_rational(x, sr_in, SR_OUT)
    b = eng.resample_rational(x, sr_in, SR_OUT)
    np.testing.assert_array_equal(a, b)
    dev = torch.device("cuda", eng.device)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(x).to(dev)
        yd = torch.full((2, a.shape[1]), float("nan"), dtype=torch.float32, device=dev)
        eng.resample_rational_dev(xd.data_ptr(), 2, n, sr_in, SR_OUT, yd.data_ptr(), a.shape[1], stream=stream.cuda_stream)
        stream.synchronize()
    np.testing.assert_array_equal(yd.cpu().numpy(), a)
    import audio_separator_amd as A
    with pytest.raises(A.AsxError, match="n_out"):
        eng.resample_rational_dev(xd.data_ptr(), 2, n, sr_in, SR_OUT, yd.data_ptr(), a.shape[1] - 1, stream=stream.cuda_stream)
