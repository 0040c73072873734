"""TEST INFRASTRUCTURE ONLY: float64 statements of Ensembler.ensemble and spec_utils.invert_stem for tests/test_gpu_ensemble_kernels.py,
written directly on np.fft.rfft / irfft over explicit frames (librosa semantics: n_fft 2048, hop 1024, periodic Hann, centre, zero
padding) and independent of oracle/ensemble_oracle.py; tests/test_host_ensemble_ref.py holds the two against each other.

Error measure of the spectral algorithms: the istft divides sample j by the squared-window sum wss_j of the frames that cover it.  In the
interior wss lies in [0.5, 1]; in the last hop of a `length=N` result it falls to ~5e-12, so an inverse-transform error e in the
frames becomes e * sum(w_t) / sum(w_t^2) <= e * sqrt(2 / wss_j) in the sample.  scaled_err weighs every sample's error by
sqrt(min(wss_j, 1)): about 1 in the interior, the conditioning of the division in the tail.
"""
import numpy as np

N_FFT, HOP = 2048, 1024
NB = N_FFT // 2 + 1
ALGORITHMS = ("avg_wave", "median_wave", "min_wave", "max_wave", "avg_fft", "median_fft", "min_fft", "max_fft", "uvr_max_spec",
              "uvr_min_spec", "ensemble_wav")
SPECTRAL = ("avg_fft", "median_fft", "min_fft", "max_fft", "uvr_max_spec", "uvr_min_spec")
SELECTING = ("min_fft", "max_fft", "uvr_max_spec", "uvr_min_spec")
MUTANTS = ("min_fft_last", "uvr_max_spec_first", "median_fft_mag")


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def n_frames(n):
    return 1 + n // HOP


def stft(x):
    """x [..., n] -> complex128 [..., 1025, T]: frame t is the windowed samples t * 1024 - 1024 .. t * 1024 + 1023 (zeros outside)"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    T = n_frames(n)
    xp = np.zeros(x.shape[:-1] + (N_FFT + HOP * (T - 1) + N_FFT,))
    xp[..., N_FFT // 2: N_FFT // 2 + n] = x
    w = window()
    fr = np.stack([xp[..., t * HOP: t * HOP + N_FFT] * w for t in range(T)], axis=-1)   # [..., 2048, T]
    return np.fft.rfft(fr, axis=-2)


def _wss_padded(T):
    ss = np.zeros(N_FFT + HOP * (T - 1))
    w2 = window() ** 2
    for t in range(T):
        ss[t * HOP: t * HOP + N_FFT] += w2
    return ss


def wss(n, n_out):
    """squared-window sum of the T = 1 + n // 1024 frames at output samples 0 .. n_out - 1"""
    return _wss_padded(n_frames(n))[N_FFT // 2: N_FFT // 2 + n_out]


def istft(S, n_out):
    """S [..., 1025, T] -> [..., n_out]: windowed inverse frames overlap-added, divided by the squared-window sum where it is not tiny"""
    S = np.asarray(S, np.complex128)
    T = S.shape[-1]
    fr = np.fft.irfft(S, n=N_FFT, axis=-2) * window()[:, None]
    y = np.zeros(S.shape[:-2] + (N_FFT + HOP * (T - 1),))
    for t in range(T):
        y[..., t * HOP: t * HOP + N_FFT] += fr[..., t]
    ss = _wss_padded(T)
    ok = ss > np.finfo(np.float64).tiny
    y[..., ok] /= ss[ok]
    assert N_FFT // 2 + n_out <= y.shape[-1]
    return y[..., N_FFT // 2: N_FFT // 2 + n_out]


def roundtrip(x, n_out=None):
    x = np.asarray(x, np.float64)
    return istft(stft(x), x.shape[-1] if n_out is None else n_out)


def _select(S, take):
    """walk the members in order; member k replaces the current choice where take(|S_k|, |current|)"""
    cur = S[0].copy()
    for k in range(1, len(S)):
        m = take(np.abs(S[k]), np.abs(cur))
        cur[m] = S[k][m]
    return cur


def ensemble(waves, alg, weights=None, mutant=None):
    """waves: K arrays [2, n] of one length -> float64 [2, n] ([2, 1024 * (n // 1024)] for uvr_*).  `mutant` (one of MUTANTS) swaps in a
    deliberately wrong rule for the algorithm it names; only the host test uses it."""
    a = np.stack([np.asarray(w, np.float64) for w in waves])
    K, _, n = a.shape
    if K == 1:
        return a[0]
    wt = np.ones(K) if weights is None else np.asarray(weights, np.float64)
    assert mutant is None or (mutant in MUTANTS and mutant.startswith(alg))
    if alg == "avg_wave":
        return np.tensordot(wt, a, 1) / wt.sum()
    if alg == "median_wave":
        return np.median(a, axis=0)
    if alg == "min_wave":
        return _select(a, lambda new, cur: new < cur)      # the first minimum of |x| stays
    if alg == "max_wave":
        return _select(a, lambda new, cur: new > cur)
    if alg == "ensemble_wav":                              # each channel whole from the member with the smallest mean |x|, the first such
        out = np.empty((2, n))
        for c in range(2):
            best = 0
            for k in range(1, K):
                if np.abs(a[k, c]).mean() < np.abs(a[best, c]).mean():
                    best = k
            out[c] = a[best, c]
        return out
    if alg not in SPECTRAL:
        raise ValueError(alg)
    S = stft(a)                                            # [K, 2, 1025, T]
    n_out = n
    if alg == "avg_fft":
        E = np.tensordot(wt, S, 1) / wt.sum()
    elif alg == "median_fft":
        if mutant == "median_fft_mag":                     # the member of median magnitude (mean of the two middle ones for even K)
            order = np.argsort(np.abs(S), axis=0, kind="stable")
            Ss = np.take_along_axis(S, order, 0)
            E = Ss[K // 2] if K & 1 else 0.5 * (Ss[K // 2 - 1] + Ss[K // 2])
        else:
            E = np.median(S.real, axis=0) + 1j * np.median(S.imag, axis=0)
    elif alg == "min_fft":
        E = _select(S, (lambda new, cur: new <= cur) if mutant == "min_fft_last" else (lambda new, cur: new < cur))
    elif alg == "max_fft":
        E = _select(S, lambda new, cur: new > cur)
    else:
        n_out = HOP * (n // HOP)                           # no length argument: hop * (T - 1) samples
        if alg == "uvr_min_spec":
            E = _select(S, lambda new, cur: new <= cur)    # the last minimum wins
        else:
            E = _select(S, (lambda new, cur: new > cur) if mutant == "uvr_max_spec_first" else (lambda new, cur: new >= cur))
    return istft(E, n_out)


def invert_stem(mix, stem):
    """[2, n], [2, n] -> [1024 * (n // 1024), 2]: -istft(Y - max(|X|, |Y|) exp(j angle X)); angle(0) = 0"""
    X, Y = stft(mix), stft(stem)
    n = np.asarray(mix).shape[-1]
    v = Y - np.maximum(np.abs(X), np.abs(Y)) * np.exp(1j * np.angle(X))
    return -istft(v, HOP * (n // HOP)).T


def ambiguous_bins(waves, kind, delta):
    """the number of (channel, bin, frame) at which the two smallest (kind "min") or two largest ("max") member magnitudes differ by
    less than delta x the rms magnitude over all members and bins"""
    mag = np.sort(np.abs(stft(np.stack([np.asarray(w, np.float64) for w in waves]))), axis=0)
    rms = np.sqrt(np.mean(mag ** 2))
    gap = mag[1] - mag[0] if kind == "min" else mag[-1] - mag[-2]
    return int(np.count_nonzero(gap < delta * rms))


def scaled_err(got, ref, n, peak=None):
    """max_j |got - ref|_j * sqrt(min(wss_j, 1)) / max |ref| for [..., n_out] results of n-sample inputs (module docstring).  `peak`
    replaces max |ref|: a number where the reference is a cancellation to zero, or "weighted" for max_j |ref|_j * sqrt(min(wss_j, 1)).
    The weighted peak is the stricter form for the selecting algorithms at n = 1024 k - 1: their spectra are no STFT of any signal, the
    last frame does not fall off like the window, and the division by wss ~ 5e-12 leaves tail samples 1e4 x the signal, which as
    max |ref| would hide every error elsewhere; weighted, such a sample counts as the inverse-transform value it was made from."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    wgt = np.sqrt(np.minimum(wss(n, ref.shape[-1]), 1.0))
    scale = np.abs(ref).max() if peak is None else (np.abs(ref) * wgt).max() if isinstance(peak, str) else peak
    return float((np.abs(got - ref) * wgt).max() / max(scale, 1e-300))


def members(seed, n, k, scale=0.3):
    """K float32 members [2, n], drawn in order from one generator"""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((2, n)) * scale).astype(np.float32) for _ in range(k)]


# Exact ties: negation and scaling by two commute with every rounding of a transform, so |X| of w and -w (2w and -2w) are equal bit for
# bit in any precision.  (multipliers of w per member, algorithm, multiplier of the member that must win)
TIE_N = 3000
TIES = (((1, -1, 2), "min_fft", 1), ((1, -1, 2), "uvr_min_spec", -1), ((1, -1, 2), "median_fft", 1),
        ((1, 2, -2), "max_fft", 2), ((1, 2, -2), "uvr_max_spec", -2))


def tie_members(mult, seed=7):
    w = members(seed, TIE_N, 1)[0]
    return [np.float32(m) * w for m in mult]
