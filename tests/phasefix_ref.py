"""TEST INFRASTRUCTURE ONLY: the float64 statement of the phase fix (include/asx.h) for tests/test_gpu_phasefix*.py,
written on np.fft.rfft / irfft over explicit frames; tests/test_host_phasefix_ref.py pins it to torch.stft / torch.istft.

Per channel: librosa-style STFTs T, S (n_fft 2048, hop h, periodic Hann, centred, zero padding, 1 + n // h frames) of the target (n samples)
and of the source zero-extended or cut to n; per frame and bin k with z = S conj(T):
    delta = atan2(Im z, Re z)  (0 where z == 0),   O_k = T_k (cos(w_k delta) + j sin(w_k delta)),   out = istft(O, length = n)
Only the real parts of bins 0 and 1024 enter the inverse transform (np.fft.irfft drops the others).  Re z and Im z are formed from
separately rounded products, so source = -target gives Im z = +0 exactly and delta = +pi in every bin with a non-zero target.

``precision=np.float32`` restates the rule with every array in float32 (numpy's pocketfft in single precision): the CPU figure the
bar of the GPU test is measured against."""
import numpy as np

N_FFT = 2048
NB = N_FFT // 2 + 1
HOPS = (256, 512, 1024)


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def n_frames(n, hop):
    return 1 + n // hop


def stft(x, hop, dtype=np.float64):
    """x [..., n] -> complex [..., 1025, T]: frame t is the windowed samples t * hop - 1024 .. t * hop + 1023 (zeros outside)"""
    x = np.asarray(x, dtype)
    n = x.shape[-1]
    T = n_frames(n, hop)
    xp = np.zeros(x.shape[:-1] + (N_FFT + hop * (T - 1) + N_FFT,), dtype)
    xp[..., N_FFT // 2: N_FFT // 2 + n] = x
    w = window().astype(dtype)
    fr = np.stack([xp[..., t * hop: t * hop + N_FFT] * w for t in range(T)], axis=-1)   # [..., 2048, T]
    return np.fft.rfft(fr, axis=-2)


def _wss_padded(T, hop):
    ss = np.zeros(N_FFT + hop * (T - 1))
    w2 = window() ** 2
    for t in range(T):
        ss[t * hop: t * hop + N_FFT] += w2
    return ss


def wss(n, hop):
    """squared-window sum of the 1 + n // hop frames at output samples 0 .. n - 1"""
    return _wss_padded(n_frames(n, hop), hop)[N_FFT // 2: N_FFT // 2 + n]


def istft(S, n, hop, dtype=np.float64):
    """S [..., 1025, T] -> [..., n] (librosa.istft with length = n): windowed inverse frames overlap-added, over the squared-window sum"""
    T = S.shape[-1]
    assert T == n_frames(n, hop), (T, n, hop)
    fr = np.fft.irfft(S, n=N_FFT, axis=-2).astype(dtype) * window().astype(dtype)[:, None]
    y = np.zeros(S.shape[:-2] + (N_FFT + hop * (T - 1),), dtype)
    for t in range(T):
        y[..., t * hop: t * hop + N_FFT] += fr[..., t]
    ss = _wss_padded(T, hop).astype(dtype)
    ok = ss > np.finfo(dtype).tiny
    y[..., ok] /= ss[ok]
    return y[..., N_FFT // 2: N_FFT // 2 + n]


def bin_weights(sample_rate, low_hz=500.0, high_hz=5000.0, low_weight=0.0, high_weight=0.8):
    """float32 [1025], bin by bin in Python floats (float64): f_k = k * sample_rate / 2048; low_weight below low_hz, high_weight above
    high_hz, linear in between; low_hz == high_hz: a bin exactly there takes high_weight"""
    out = np.empty(NB, np.float32)
    for k in range(NB):
        f = k * float(sample_rate) / N_FFT
        if f < low_hz:
            w = low_weight
        elif f > high_hz or f == high_hz:
            w = high_weight
        else:
            w = low_weight + (high_weight - low_weight) * (f - low_hz) / (high_hz - low_hz)
        out[k] = w
    return out


def fit_source(source, n):
    """the source [2, m] zero-extended or cut to n samples"""
    source = np.asarray(source)
    out = np.zeros((2, n), source.dtype)
    m = min(n, source.shape[1])
    out[:, :m] = source[:, :m]
    return out


def spectra(target, source, hop, dtype=np.float64):
    target = np.asarray(target, dtype)
    return stft(target, hop, dtype), stft(fit_source(np.asarray(source, dtype), target.shape[1]), hop, dtype)


def z_parts(T, S):
    """(Re z, Im z) of z = S conj(T), every product rounded on its own"""
    return S.real * T.real + S.imag * T.imag, S.imag * T.real - S.real * T.imag


def phase_fix(target, source, weights, hop=512, precision=np.float64):
    """target [2, n], source [2, m], weights [1025] -> [2, n] in ``precision``"""
    dtype = np.dtype(precision).type
    n = np.asarray(target).shape[1]
    T, S = spectra(target, source, hop, dtype)
    re, im = z_parts(T, S)
    delta = np.where((re == 0) & (im == 0), dtype(0), np.arctan2(im, re))
    ang = np.asarray(weights, dtype)[:, None] * delta
    O = T * (np.cos(ang) + 1j * np.sin(ang)).astype(T.dtype)
    return istft(O, n, hop, dtype)


def ambiguous_bins(target, source, weights, hop=512):
    """The number of (channel, bin, frame) at which rounding could turn delta from near +pi to near -pi and the result would change with
    it: w_k is not an integer, Re z < 0 and |Im z| <= 4 (|T| e_S + |S| e_T), e_X = 1e-6 x the rms bin magnitude of X.  Bins 0 and 1024
    never count (their spectra are real, and only the real part of their result is used)."""
    T, S = spectra(target, source, hop)
    re, im = z_parts(T, S)
    e_t, e_s = (1e-6 * np.sqrt(np.mean(np.abs(X) ** 2)) for X in (T, S))
    w = np.asarray(weights, np.float64)
    frac = (w != np.round(w))[:, None]
    amb = frac & (re < 0) & (np.abs(im) <= 4.0 * (np.abs(T) * e_s + np.abs(S) * e_t))
    amb[..., 0, :] = False
    amb[..., NB - 1, :] = False
    return int(np.count_nonzero(amb))


def scaled_err(got, ref, n, hop):
    """tests.ensemble_ref.scaled_err with the window sum of this hop: max_j |got - ref|_j sqrt(min(wss_j, 1)) / max |ref|.  The frames of
    hop 256 or 512 include those of hop 1024, so this weight is nowhere below that one: the measure is the stricter of the two."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    wgt = np.sqrt(np.minimum(wss(n, hop), 1.0))
    return float((np.abs(got - ref) * wgt).max() / max(np.abs(ref).max(), 1e-300))


def stems(seed, n, m=None, scale=0.3):
    """float32 target [2, n] and source [2, m]: the source is the target plus an independent part of the same size, as two models'
    takes of one stem are"""
    rng = np.random.default_rng(seed)
    m = n if m is None else m
    t = rng.standard_normal((2, n)) * scale
    s = np.zeros((2, m))
    k = min(n, m)
    s[:, :k] = 0.5 * t[:, :k]
    s += rng.standard_normal((2, m)) * scale * 0.8
    return t.astype(np.float32), s.astype(np.float32)
