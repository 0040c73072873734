"""tests/phasefix_ref.py -- the float64 statement the phase-fix kernels are tested against -- pinned to torch.stft / torch.istft in
float64 (center=True, pad_mode="constant", periodic Hann, length=n): the round trip with all weights 0, and |T| S / |S| formed with
torch with all weights 1.  The weight table at and around both cutoffs.  The float32 restatement of the rule, measured against the
float64 one over the shapes of tests/test_gpu_phasefix_kernels.py: the figure that test's bar (5e-6) is twenty times of."""
import numpy as np
import pytest
import torch

from tests import ensemble_ref as ER
from tests import phasefix_ref as R

SHAPES = (1, 511, 512, 513, 2047, 2048, 2049, 3000, 5121)


def t_stft(x, hop):
    x = torch.as_tensor(np.asarray(x, np.float64))
    return torch.stft(x, R.N_FFT, hop_length=hop, window=torch.hann_window(R.N_FFT, periodic=True, dtype=torch.float64), center=True,
                      pad_mode="constant", return_complex=True)


def cond(n, hop):
    """the weight of tests.ensemble_ref.scaled_err at this hop: the division by a window sum of ~5e-12 in the last samples of n = 1024 k - 1
    at hop 1024 turns a float64 rounding of the frames into ~1e-11 in the sample"""
    return np.sqrt(np.minimum(R.wss(n, hop), 1.0))


def t_istft(X, hop, n):
    return torch.istft(X, R.N_FFT, hop_length=hop, window=torch.hann_window(R.N_FFT, periodic=True, dtype=torch.float64), center=True,
                       length=n).numpy()


@pytest.mark.parametrize("hop", R.HOPS)
@pytest.mark.parametrize("n", (1, 513, 2049, 5121))
def test_frames_are_torch_stft(n, hop):
    t, _ = R.stems(3, n)
    X = t_stft(t, hop).numpy()
    assert X.shape == (2, R.NB, 1 + n // hop)
    assert np.abs(R.stft(t, hop) - X).max() <= 1e-12 * max(np.abs(X).max(), 1.0)


@pytest.mark.parametrize("hop", R.HOPS)
@pytest.mark.parametrize("n", SHAPES)
def test_all_weights_zero_is_the_round_trip(n, hop):
    t, s = R.stems(n, n, n + 100)
    got = R.phase_fix(t, s, np.zeros(R.NB), hop)
    want = t_istft(t_stft(t, hop), hop, n)
    assert got.shape == (2, n) and (np.abs(got - want) * cond(n, hop)).max() <= 1e-12
    assert (np.abs(got - t) * cond(n, hop)).max() <= 1e-12    # (and the round trip is the identity: every sample is covered)


@pytest.mark.parametrize("hop", R.HOPS)
@pytest.mark.parametrize("n", (513, 2048, 3000, 5121))
def test_all_weights_one_is_the_phase_swap(n, hop):
    t, s = R.stems(n + 1, n, n - 200)
    T, S = t_stft(t, hop), t_stft(R.fit_source(s, n), hop)
    assert float(S.abs().min()) > 0.0
    want = t_istft(T.abs() * S / S.abs(), hop, n)
    got = R.phase_fix(t, s, np.ones(R.NB), hop)
    assert (np.abs(got - want) * cond(n, hop)).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


def test_half_weight_halves_the_angle_and_two_doubles_it():
    """one bin, by hand: T = 1, S at +120 degrees -> w = 0.5 gives +60, w = 2 gives +240 = -120; S at -120 mirrors"""
    T = np.array([1.0 + 0j])
    for sign in (1.0, -1.0):
        S = np.array([np.exp(sign * 2j * np.pi / 3)])
        re, im = R.z_parts(T, S)
        delta = np.arctan2(im, re)
        assert abs(delta[0] - sign * 2 * np.pi / 3) < 1e-15
    # the tie: S = -T gives +pi, whatever T
    rng = np.random.default_rng(0)
    T = rng.standard_normal(1000) + 1j * rng.standard_normal(1000)
    re, im = R.z_parts(T, -T)
    assert (im == 0).all() and not np.signbit(im).any() and (np.arctan2(im, re) == np.pi).all()


def test_tie_rule_in_the_full_statement():
    t, _ = R.stems(5, 3000)
    w = np.full(R.NB, 0.5)
    T = R.stft(t, 512)
    want = R.istft(T * np.exp(0.5j * np.pi), 3000, 512)
    assert (np.abs(R.phase_fix(t, -t, w, 512) - want) * cond(3000, 512)).max() <= 1e-12


def test_weight_table_at_and_around_the_cutoffs():
    from audio_separator_amd import phasefix as P
    # 44100 Hz: bin k at k * 21.533203125 Hz; 500 Hz lies between bins 23 and 24, 5000 Hz between 232 and 233
    w = P.bin_weights(44100)
    assert w.dtype == np.float32 and w.shape == (1025,)
    assert (w[:24] == 0).all() and w[24] > 0 and (w[233:] == np.float32(0.8)).all() and w[232] < np.float32(0.8)
    assert np.array_equal(w, R.bin_weights(44100))
    f = np.arange(1025) * 44100 / 2048
    line = 0.8 * (f[24:233] - 500.0) / 4500.0
    assert np.abs(w[24:233] - line).max() <= 2.0 ** -24
    # 32768 Hz: bin k at exactly 16 k Hz, so cutoffs can sit on bins
    w = P.bin_weights(32768, low_hz=160, high_hz=320, low_weight=-0.5, high_weight=2.0)
    assert np.array_equal(w, R.bin_weights(32768, 160, 320, -0.5, 2.0))
    assert w[9] == -0.5 and w[10] == -0.5 and w[11] == np.float32(-0.5 + 2.5 / 10) and w[15] == 0.75 and w[19] == np.float32(2.0 - 2.5 / 10)
    assert w[20] == 2.0 and w[21] == 2.0
    # low_hz == high_hz: below low, at and above high
    w = P.bin_weights(32768, low_hz=160, high_hz=160, low_weight=0.25, high_weight=1.5)
    assert np.array_equal(w, R.bin_weights(32768, 160, 160, 0.25, 1.5))
    assert (w[:10] == 0.25).all() and (w[10:] == 1.5).all()
    w = P.bin_weights(32768, low_hz=150, high_hz=150, low_weight=0.25, high_weight=1.5)       # between bins 9 and 10
    assert (w[:10] == 0.25).all() and (w[10:] == 1.5).all()
    # cutoffs outside the band
    assert (P.bin_weights(44100, 30000, 40000, 0.3, 0.9) == np.float32(0.3)).all()
    assert (P.bin_weights(44100, 0, 0, 0.3, 0.9) == np.float32(0.9)).all()
    with pytest.raises(ValueError, match="low_hz"):
        P.bin_weights(44100, 600, 500)
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="finite"):
            P.bin_weights(44100, high_weight=bad)
        with pytest.raises(ValueError, match="finite"):
            P.bin_weights(44100, low_weight=bad)


def test_ambiguous_bins_counts_what_it_says():
    t, s = R.stems(1, 3000)
    ramp = R.bin_weights(44100)
    assert R.ambiguous_bins(t, -t, np.full(R.NB, 0.5)) > 1000           # every bin is a tie
    assert R.ambiguous_bins(t, -t, np.ones(R.NB)) == 0                  # integer weights: either sign gives the same result
    assert R.ambiguous_bins(t, t, np.full(R.NB, 0.5)) == 0              # Re z > 0 everywhere
    a = R.ambiguous_bins(t, s, ramp)
    assert 0 <= a < 10


def test_float32_statement_against_float64(capsys):
    """What a float32 CPU implementation of the rule needs, in the GPU test's measure, over its shapes at hop 512 and 1024 with the
    default ramp.  The bar of tests/test_gpu_phasefix_kernels.py is 5e-6."""
    from tests import phasefix_cases as PC
    assert PC.SHAPES == SHAPES
    ramp = R.bin_weights(44100)
    worst = 0.0
    for hop in (512, 1024):
        for n in SHAPES:
            assert PC.unambiguous(n, n, hop), "the seed no longer gives stems without near-ties: the comparison would not be defined"
            t, s = PC.case(n, n, hop)
            ref = PC.reference(n, n, hop, "ramp")
            got = R.phase_fix(t, s, ramp, hop, precision=np.float32)
            assert got.dtype == np.float32
            e = max(ER.scaled_err(got, ref, n), R.scaled_err(got, ref, n, hop))
            worst = max(worst, e)
    with capsys.disabled():
        print(f"\nPHASEFIX float32 numpy statement, worst scaled_err over {len(SHAPES)} shapes x hop 512, 1024: {worst:.3e}")
    assert worst <= 5e-6 / 4
