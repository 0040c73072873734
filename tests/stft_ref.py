"""Float64 reference of the STFT / iSTFT launches (asx_op_stft, asx_op_istft, asx_op_ht_spec, asx_op_ht_ispec), written from the
formulas: framing, the engine's fp32 window table read as float64, numpy's float64 rfft / irfft, overlap-add and the float64 envelope
of the same window.  Also the error measures of tests/test_gpu_stft_kernels.py and the fp32 yardstick e32 its bar is made of.

Measures
  forward: the worst element (real and imaginary parts apart) of |kernel - f64| / P, P = the largest |X64| over bins 0 .. n/2 of that
           element's frame, before cropping to dim_f or zeroing the low bins.  NaN counts as infinite.
  inverse: the worst sample of |kernel - f64| / s_j, s_j = (sum_t peak_t |w[m - t hop]|) / env[m], peak_t the largest |irfft64| of
           frame t before the window (times the chunk window where one is applied; plus |time branch| for the Demucs inverse, whose
           output is the sum of the two and is rounded once more after the sum).
  e32:     the same measure for a plain fp32 evaluation on the CPU: torch.fft.rfft of the fp32-rounded windowed frames; torch.fft.irfft,
           fp32 window, fp32 overlap-add in increasing t, fp32 divide.
  bar:     8 x max(e32, 2^-23); nothing in it comes from a kernel's output.
Frames whose float64 spectrum is identically zero, and samples with s_j = 0, have no scale: they must come back as exact zeros and are
reported apart (`zero_bad`), never dropped."""
import numpy as np
import torch

BAR_FACTOR = 8.0
EPS_FLOOR = 2.0 ** -23


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def hann_table(n_fft, win_length=0):
    """The engine's default window: periodic Hann over win_length, zero padded to n_fft at both ends, rounded to fp32."""
    wl = win_length if 0 < win_length < n_fft else n_fft
    off = (n_fft - wl) // 2
    w = np.zeros(n_fft, np.float64)
    w[off:off + wl] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(wl, dtype=np.float64) / wl)
    return w.astype(np.float32)


def hamming_table(n_fft):
    """torch.hamming_window(n_fft) (periodic), fp32 -- a table for asx_set_stft_window."""
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)).astype(np.float32)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def spec_index(layout, B, S, T, F, subbands=0, bstride=0):
    """Flat float indices [B, S, 2 (channel), T, F, 2 (re, im)] of the spectrum of (batch item, stem) in the three layouts
    (csrc/kernels_fft.h).  Layout 2 has no stem axis of its own (S spectra share the item's row; S must be 1 here)."""
    b = np.arange(B).reshape(B, 1, 1, 1, 1, 1)
    s = np.arange(S).reshape(1, S, 1, 1, 1, 1)
    ch = np.arange(2).reshape(1, 1, 2, 1, 1, 1)
    t = np.arange(T).reshape(1, 1, 1, T, 1, 1)
    k = np.arange(F).reshape(1, 1, 1, 1, F, 1)
    ri = np.arange(2).reshape(1, 1, 1, 1, 1, 2)
    if layout == 0:
        assert S == 1
        return (((b * 4 + ch * 2 + ri) * F + k) * T + t) + 0 * s
    if layout == 1:
        kb = max(subbands, 1)
        fs = F // kb
        bst = bstride or S * 4 * T * F
        return b * bst + ((((s * 4 + ch * 2 + ri) * kb + k // fs) * T + t) * fs + k % fs)
    assert S == 1
    return ((((b * T + t) * F + k) * 2 + ch) * 2 + ri) + 0 * s


def mask_index(B, S, T, F):
    """[B, S, 2, T, F, 2] indices into the Roformer mask [b, s, t, f, channel, (re, im)]."""
    b = np.arange(B).reshape(B, 1, 1, 1, 1, 1)
    s = np.arange(S).reshape(1, S, 1, 1, 1, 1)
    ch = np.arange(2).reshape(1, 1, 2, 1, 1, 1)
    t = np.arange(T).reshape(1, 1, 1, T, 1, 1)
    k = np.arange(F).reshape(1, 1, 1, 1, F, 1)
    ri = np.arange(2).reshape(1, 1, 1, 1, 1, 2)
    return (((((b * S + s) * T + t) * F + k) * 2 + ch) * 2 + ri)


def as_complex(flat, idx):
    v = np.asarray(flat).reshape(-1)[idx]
    return v[..., 0].astype(np.float64) + 1j * v[..., 1].astype(np.float64)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
def chunk_positions(n_fft, hop, T, C):
    """[T, n_fft] chunk positions of the frame elements: centre padding of n_fft / 2, reflected once at either chunk end."""
    q = np.arange(T, dtype=np.int64)[:, None] * hop + np.arange(n_fft, dtype=np.int64)[None, :] - n_fft // 2
    q = np.where(q < 0, -q, q)
    q = np.where(q >= C, 2 * (C - 1) - q, q)
    assert q.min() >= 0 and q.max() < C
    return q


def frames_chunks(wave, n_fft, hop, T):
    """wave [B, 2, C] -> frames [B, 2, T, n_fft] (fp32 values)."""
    return wave[:, :, chunk_positions(n_fft, hop, T, wave.shape[-1])]


def frames_song(songs, song_of, starts, front, C, n_fft, hop, T):
    """Song mode: chunk i is a window of songs[song_of[i]] ([2, N]) starting at padded position starts[i]; padded position j is
    song[j - front] inside the song and 0 elsewhere."""
    q = chunk_positions(n_fft, hop, T, C)
    out = np.zeros((len(starts), 2, T, n_fft), np.float32)
    for i, (s, st) in enumerate(zip(song_of, starts)):
        song = songs[s]
        j = int(st) + q - front
        ok = (j >= 0) & (j < song.shape[1])
        out[i] = np.where(ok[None], song[:, np.clip(j, 0, song.shape[1] - 1)], 0.0)
    return out


def frames_demucs(seg, nfft, el=0, lv=None):
    """HTDemucs / HDemucs _spec framing: seg [B, 2, L] zero extended to lv samples with el in front (pad1d), reflected by 3 hop / 2 on
    the left and up to a whole number of hops on the right; frame t starts at t hop - 3 hop / 2."""
    L = seg.shape[-1]
    lv = L if lv is None else lv
    hop = nfft // 4
    T = -(-L // hop)
    q = np.arange(T, dtype=np.int64)[:, None] * hop + np.arange(nfft, dtype=np.int64)[None, :] - hop // 2 * 3 + el
    q = np.where(q < 0, -q, q)
    q = np.where(q >= lv, 2 * (lv - 1) - q, q)
    assert q.min() >= 0 and q.max() < lv
    q = q - el
    ok = (q >= 0) & (q < L)
    return np.where(ok[None, None], seg[:, :, np.clip(q, 0, L - 1)], np.float32(0))


def demucs_extension(L, nfft):
    """(el, lv) of pad1d's zero extension for a segment of L samples (hdemucs.py pad1d: inputs no longer than the reflect pad)."""
    hop = nfft // 4
    T = -(-L // hop)
    left = hop // 2 * 3
    right = left + T * hop - L
    mx = max(left, right)
    if L > mx:
        return 0, L
    extra = mx - L + 1
    er = min(right, extra)
    return extra - er, L + extra


def forward64(frames, window, scale=1.0):
    """frames [..., T, n] fp32, window [n] fp32 -> (X64 [..., T, n/2 + 1], P [..., T], e32) with X64 = scale * rfft(frames * window)."""
    f64 = frames.astype(np.float64) * window.astype(np.float64)
    X = np.fft.rfft(f64, axis=-1) * scale
    P = np.abs(X).max(axis=-1)
    f32 = torch.from_numpy(np.ascontiguousarray(frames, np.float32)) * torch.from_numpy(window.astype(np.float32))
    X32 = torch.fft.rfft(f32, dim=-1) * torch.tensor(scale, dtype=torch.float32)
    X32 = X32.numpy()
    d = np.maximum(np.abs(X32.real.astype(np.float64) - X.real), np.abs(X32.imag.astype(np.float64) - X.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(P[..., None] > 0, d / P[..., None], 0.0)
    return X, P, float(r.max())


def bar(e32):
    return BAR_FACTOR * max(e32, EPS_FLOOR)


def measure(got, want, scale):
    """(worst |got - want| / scale over elements with scale > 0, elements with scale == 0 that are not exact zeros).  got / want real
    arrays of one shape, scale broadcastable.  NaN counts as infinite."""
    got = np.asarray(got, np.float64)
    scale = np.broadcast_to(scale, got.shape)
    d = np.abs(got - want)
    d = np.where(np.isnan(d), np.inf, d)
    pos = scale > 0
    worst = float((d[pos] / scale[pos]).max()) if pos.any() else 0.0
    zero_bad = int(np.count_nonzero(got[~pos] != 0) + np.count_nonzero(np.isnan(got[~pos])))
    return worst, zero_bad


def forward_measure(got_c, X, P, dim_f, zero_low=0):
    """got_c complex [..., T, dim_f] (kernel), X [..., T, n/2 + 1] (float64, already scaled and signed)."""
    want = X[..., :dim_f].copy()
    want[..., :zero_low] = 0
    # the zeroed low bins have a scale (their frame's) but must be exact zeros all the same: measured with the rest, and exactly here
    w1, z1 = measure(got_c.real, want.real, P[..., None])
    w2, z2 = measure(got_c.imag, want.imag, P[..., None])
    low = got_c[..., :zero_low]
    z3 = int(np.count_nonzero(low.real != 0) + np.count_nonzero(low.imag != 0) + np.count_nonzero(np.isnan(low.real) | np.isnan(low.imag)))
    return max(w1, w2), z1 + z2 + z3


# ---- inverse -----------------------------------------------------------------------------------------------------------------------
def c2r_spectrum(X, n_fft):
    """X [..., dim_f] complex -> [..., n/2 + 1]: bins >= dim_f zero, the imaginary parts of DC and Nyquist ignored."""
    Z = np.zeros(X.shape[:-1] + (n_fft // 2 + 1,), np.complex128)
    Z[..., :X.shape[-1]] = X
    Z[..., 0] = Z[..., 0].real
    Z[..., -1] = Z[..., -1].real
    return Z


def envelope(window, hop, T):
    n = window.size
    env = np.zeros(n + hop * (T - 1), np.float64)
    w2 = window.astype(np.float64) ** 2
    for t in range(T):
        env[t * hop:t * hop + n] += w2
    return env


def envelope32(window, hop, T):
    n = window.size
    env = np.zeros(n + hop * (T - 1), np.float32)
    w2 = window.astype(np.float32) * window.astype(np.float32)
    for t in range(T):
        env[t * hop:t * hop + n] += w2
    return env


def inverse64(Z, window, hop, C, scale=1.0, n_act=None, offset=None, env=None, env32=None):
    """Z [R, T, n/2 + 1] (c2r-clean) -> (out64 [R, C], s [R, C], e32): irfft, x scale, window, overlap-add, / envelope, samples
    [offset, offset + C) of the padded domain (default n_fft / 2), the chunk window np.hanning(n_act[r]) (n_act[r] >= 0) and zeros
    behind it.  env / env32: the envelopes to divide by (default: of these T frames)."""
    R, T, _ = Z.shape
    n = window.size
    offset = n // 2 if offset is None else offset
    w64 = window.astype(np.float64)
    y = np.fft.irfft(Z, n=n, axis=-1) * scale
    peak = np.abs(y).max(axis=-1)                                      # [R, T]
    env = envelope(window, hop, T) if env is None else env
    acc = np.zeros((R, n + hop * (T - 1)), np.float64)
    sc = np.zeros_like(acc)
    for t in range(T):
        acc[:, t * hop:t * hop + n] += y[:, t] * w64
        sc[:, t * hop:t * hop + n] += peak[:, t, None] * np.abs(w64)
    sl = slice(offset, offset + C)
    e = env[sl] if env.ndim == 1 else env[:, sl]
    out = acc[:, sl] / e
    s = sc[:, sl] / e
    # fp32 yardstick
    y32 = torch.fft.irfft(torch.from_numpy(Z.astype(np.complex64)), n=n, dim=-1) * torch.tensor(scale, dtype=torch.float32)
    fr32 = (y32 * torch.from_numpy(window.astype(np.float32))).numpy()
    acc32 = np.zeros((R, n + hop * (T - 1)), np.float32)
    for t in range(T):
        acc32[:, t * hop:t * hop + n] += fr32[:, t]
    env32 = envelope32(window, hop, T) if env32 is None else env32
    e32v = env32[sl] if env32.ndim == 1 else env32[:, sl]
    out32 = (acc32[:, sl] / e32v).astype(np.float64)
    if n_act is not None:
        for r, na in enumerate(n_act):
            if na >= 0:
                h = np.zeros(C, np.float64)
                h[:min(na, C)] = np.hanning(na)[:C]
                out[r] *= h
                s[r] *= h
                out32[r] = (out32[r] * h).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r32 = np.where(s > 0, np.abs(out32 - out) / s, 0.0)
    return out, s, float(r32.max())


# ---- Demucs ------------------------------------------------------------------------------------------------------------------------
def mean_std(acc, n):
    """(mean, std) [B] in float64 of the (sum, sum of squares) pairs over n values each, unbiased like torch.std."""
    acc = np.asarray(acc, np.float64)
    m = acc[:, 0] / n
    var = np.maximum((acc[:, 1] - n * m * m) / (n - 1.0), 0.0)
    return m, np.sqrt(var)


def demucs_env(window, hop):
    """[hop] sum over the n_fft / hop frames covering a sample of w^2 (torch.istft counts the zero frames either side too)."""
    return (window.astype(np.float64) ** 2).reshape(-1, hop).sum(axis=0)


def demucs_inverse64(x, nfft, acc_f, n_stat, xt, acc_t, L, window=None):
    """x [B, T, nfft / 2, 4 S] fp32, xt [B, L, 2 S] fp32 -> (out64 [B, S, 2, L], s, e32): X = x std + mean, Nyquist 0, irfft x sqrt(nfft),
    periodic Hann, overlap-add from 3 hop / 2 inside the first frame, / envelope, + xt std_t + mean_t."""
    B, T, nh, c4 = x.shape
    S = c4 // 4
    hop = nfft // 4
    w = hann_table(nfft) if window is None else window
    mean, std = mean_std(acc_f, n_stat)
    X = x.astype(np.float64).reshape(B, T, nh, S, 2, 2) * std[:, None, None, None, None, None] + mean[:, None, None, None, None, None]
    Xc = (X[..., 0] + 1j * X[..., 1]).transpose(0, 3, 4, 1, 2).reshape(B * S * 2, T, nh)
    Z = c2r_spectrum(Xc, nfft)
    env_h = demucs_env(w, hop)
    n_pad = nfft + hop * (T - 1)
    env = np.tile(env_h, -(-n_pad // hop))[:n_pad]
    env32_h = np.zeros(hop, np.float32)
    w32 = w.astype(np.float32).reshape(-1, hop)
    for i in range(nfft // hop - 1, -1, -1):
        env32_h += w32[i] * w32[i]
    env32 = np.tile(env32_h, -(-n_pad // hop))[:n_pad]
    # fp32 de-standardisation for the yardstick
    m32, s32 = mean.astype(np.float32), std.astype(np.float32)
    X32 = x.reshape(B, T, nh, S, 2, 2) * s32[:, None, None, None, None, None] + m32[:, None, None, None, None, None]
    Xc32 = (X32[..., 0] + 1j * X32[..., 1]).transpose(0, 3, 4, 1, 2).reshape(B * S * 2, T, nh)
    Z32 = c2r_spectrum(Xc32.astype(np.complex128), nfft)
    out, s, _ = inverse64(Z, w, hop, L, scale=np.sqrt(float(nfft)), offset=hop // 2 * 3, env=env, env32=env32)
    y32 = torch.fft.irfft(torch.from_numpy(Z32.astype(np.complex64)), n=nfft, dim=-1) * torch.tensor(np.sqrt(float(nfft)), dtype=torch.float32)
    fr32 = (y32 * torch.from_numpy(w.astype(np.float32))).numpy()
    acc32 = np.zeros((B * S * 2, n_pad), np.float32)
    for t in range(T):
        acc32[:, t * hop:t * hop + nfft] += fr32[:, t]
    sl = slice(hop // 2 * 3, hop // 2 * 3 + L)
    out32 = acc32[:, sl] / env32[sl]
    mt, st = mean_std(acc_t, 2.0 * L)
    tv = xt.astype(np.float64) * st[:, None, None] + mt[:, None, None]                 # [B, L, 2 S]
    tv = tv.transpose(0, 2, 1).reshape(B * S * 2, L)
    tv32 = (xt * st.astype(np.float32)[:, None, None] + mt.astype(np.float32)[:, None, None]).transpose(0, 2, 1).reshape(B * S * 2, L)
    total = out + tv
    s = s + np.abs(tv)
    total32 = (tv32 + out32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r32 = np.where(s > 0, np.abs(total32 - total) / s, 0.0)
    return total.reshape(B, S, 2, L), s.reshape(B, S, 2, L), float(r32.max())
