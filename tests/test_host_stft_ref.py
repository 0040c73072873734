"""The float64 STFT / iSTFT reference of tests/stft_ref.py against torch.stft / torch.istft in float64 (the generic conventions: window
functions, win_length < n_fft, normalized, hop 441) and against oracle/demucs_oracle.py's _spec / _ispec (the Demucs ones), to 1e-12 of
the peak; and the inverse cases of tests/stft_cases.py: no owned sample divides by a vanishing envelope.  No GPU."""
import types

import numpy as np
import pytest
import torch

from tests import stft_cases as K
from tests import stft_ref as R

TOL = 1e-12


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


GENERIC = [  # n_fft, hop, win_length, window, normalized, T
    (96, 24, 0, None, False, 6), (64, 16, 48, None, False, 6), (64, 16, 0, "hamming", False, 6), (2048, 441, 0, None, True, 8),
    (2048, 441, 0, None, False, 8), (20, 5, 0, None, False, 6)]


@pytest.mark.parametrize("n,hop,wl,win,normalized,T", GENERIC)
def test_generic_reference_matches_torch(n, hop, wl, win, normalized, T):
    rng = np.random.default_rng(n + hop)
    C = hop * (T - 1)
    w = R.hamming_table(n) if win == "hamming" else R.hann_table(n, wl)
    # the table is torch's window over win_length, zero padded to n_fft at both ends
    tw = torch.hamming_window(n, dtype=torch.float64) if win == "hamming" else torch.hann_window(wl or n, dtype=torch.float64)
    pad = (n - tw.numel()) // 2
    assert np.array_equal(w, torch.nn.functional.pad(tw, (pad, n - tw.numel() - pad)).float().numpy())
    w64 = torch.from_numpy(w.astype(np.float64))
    wave = rng.standard_normal((3, 2, C)).astype(np.float32)
    X, P, e32 = R.forward64(R.frames_chunks(wave, n, hop, T), w, n ** -0.5 if normalized else 1.0)
    ref = torch.stft(torch.from_numpy(wave).double().reshape(6, C), n, hop, window=w64, center=True, pad_mode="reflect", normalized=normalized,
                     return_complex=True).numpy().reshape(3, 2, n // 2 + 1, T).transpose(0, 1, 3, 2)
    assert rel(X, ref) < TOL and e32 < 1e-5 and np.all(P > 0)
    # inverse: DC and Nyquist carry imaginary parts the c2r transform ignores
    Zin = rng.standard_normal((4, T, n // 2 + 1)) + 1j * rng.standard_normal((4, T, n // 2 + 1))
    out, s, e32 = R.inverse64(R.c2r_spectrum(Zin, n), w, hop, C, scale=n ** 0.5 if normalized else 1.0)
    Zc = R.c2r_spectrum(Zin, n)
    ref = torch.istft(torch.from_numpy(Zc.transpose(0, 2, 1).copy()), n, hop, window=w64, center=True, normalized=normalized, length=C).numpy()
    assert rel(out, ref) < TOL and e32 < 1e-5
    assert np.all(s > 0) and np.all(np.abs(out) <= s * (1 + 1e-12))


def test_dim_f_crop_and_chunk_window():
    """bins >= dim_f are zero; the chunk window is np.hanning(n_act) over the first n_act samples and zero behind them"""
    rng = np.random.default_rng(3)
    n, hop, T, F = 96, 24, 6, 20
    C = hop * (T - 1)
    w = R.hann_table(n)
    X = rng.standard_normal((2, T, F)) + 1j * rng.standard_normal((2, T, F))
    Z = R.c2r_spectrum(X, n)
    assert np.all(Z[..., F:] == 0) and np.all(Z[..., 0].imag == 0) and np.array_equal(Z[..., 1:F], X[..., 1:])
    plain, s, _ = R.inverse64(Z, w, hop, C)
    win, sw, _ = R.inverse64(Z, w, hop, C, n_act=[70, -1])
    h = np.zeros(C)
    h[:70] = np.hanning(70)
    assert np.allclose(win[0], plain[0] * h, rtol=1e-14, atol=0) and np.array_equal(win[1], plain[1]) and np.all(sw[0][70:] == 0)


@pytest.mark.parametrize("nfft,L", [(4096, 7 * 1024 + 333), (1024, 2000), (1024, 877), (1024, 100), (1024, 3)])
def test_demucs_reference_matches_oracle(nfft, L):
    from oracle import demucs_oracle as O
    cfg = types.SimpleNamespace(nfft=nfft, hop=nfft // 4)
    rng = np.random.default_rng(L)
    seg = rng.standard_normal((2, 2, L)).astype(np.float32)
    hop = nfft // 4
    T = -(-L // hop)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        w64 = torch.hann_window(nfft).numpy()
        z = O._spec(torch.from_numpy(seg).double(), cfg).numpy()                           # [B, 2, F, T]
        el, lv = R.demucs_extension(L, nfft)
        X, _, _ = R.forward64(R.frames_demucs(seg, nfft, el, lv), w64, nfft ** -0.5)
        assert z.shape == (2, 2, nfft // 2, T) and rel(X[..., :-1], z.transpose(0, 1, 3, 2)) < TOL
        # inverse: mean 0 / std 1 and no time branch leave _ispec alone
        S = 2
        x = rng.standard_normal((2, T, nfft // 2, 4 * S)).astype(np.float32)
        zc = x.astype(np.float64).reshape(2, T, nfft // 2, S, 2, 2)
        zc = (zc[..., 0] + 1j * zc[..., 1]).transpose(0, 3, 4, 2, 1)                         # [B, S, 2, F, T]
        zc[..., 0, :] = zc[..., 0, :].real                                                    # torch.istft wants a real DC bin
        ref = O._ispec(torch.from_numpy(zc.copy()), L, cfg).numpy()
        n_stat = 1000.0
        acc_f = np.array([[0.0, n_stat - 1.0]] * 2)
        out, s, _ = R.demucs_inverse64(x, nfft, acc_f, n_stat, np.zeros((2, L, 2 * S), np.float32), np.zeros((2, 2)), L, window=w64)
        assert rel(out, ref) < TOL
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("name", [c["name"] for c in K.INV])
def test_inverse_cases_divide_by_a_sound_envelope(name):
    c = K.BY_NAME[name]
    env = R.envelope(K.window_of(c), c["hop"], c["T"])
    own = env[c["n_fft"] // 2:c["n_fft"] // 2 + c["C"]]
    assert own.size == c["C"] and own.min() >= 1e-3 * env.max(), (name, own.min(), env.max())
    assert c["C"] <= c["hop"] * (c["T"] - 1)


def test_demucs_envelope_is_sound():
    for nfft in (1024, 4096):
        e = R.demucs_env(R.hann_table(nfft), nfft // 4)
        assert e.min() >= 1e-3 * e.max()


def test_case_tables_name_every_kernel():
    fwd = {c["expect"][0] for c in K.FWD} | {"stft_pool" if c["mode"] == "pool" else "stft" for c in K.FWD if c["generic"]}
    inv = {c["expect"][0] for c in K.INV}
    assert fwd == {"stft", "stft_pool", "stft3", "stft3_pool", "stft3p", "stft3p_pool"} and inv == {"istft+ola", "istft3", "istft3p"}
    assert any(c["expect"][1] for c in K.INV)
