"""The ensemble and invert_stem kernels (csrc/kernels_ens.h, csrc/engine_ens.h) through Engine.ensemble / Engine.invert_stem against
the float64 statements of tests/ensemble_ref.py: at exact ties, at every K the engine builds (2 .. 8), at frame edges (N = 1024 k,
1024 k - 1, one frame, shorter than one hop), with weights, ragged members, silent frames, and at the limits (K = 1, K = 9, N = 0).

Spectral algorithms and invert_stem: BAR = 5e-6 in ensemble_ref.scaled_err, the bar of tests/test_gpu_ensemble.py, over the plain peak
and over the weighted peak (ensemble_ref.scaled_err; the weighted form is the stricter one at N = 1024 k - 1).  It is about 20x what a
float32 CPU implementation needs (2.4e-7, tests/test_host_ensemble_ref.py) and is not fitted to the kernel.  The selecting algorithms
are compared only on inputs on which the float64 reference itself shows no bin where two candidates are closer than 2e-5 of the rms
magnitude (about 30x the float32 magnitude error of FFT-2048 plus hypotf), or on exact ties, where the tie rule alone decides.
Wave-domain algorithms: bit for bit against numpy float32; avg_wave against float64 within (K + 1) roundings.

Worst scaled_err measured on an MI355X over this file, plain / weighted peak (the float32 CPU oracle on the same inputs beside it):
    avg_fft       2.1e-7 / 2.1e-7  (2.0e-7)        max_fft       1.8e-7 / 2.4e-7  (2.2e-7)
    median_fft    1.8e-7 / 3.4e-7  (2.0e-7)        uvr_max_spec  2.2e-7 / 2.4e-7  (1.9e-7)
    min_fft       2.7e-7 / 3.5e-7  (2.0e-7)        uvr_min_spec  2.8e-7 / 3.7e-7  (2.2e-7)
    invert_stem   3.1e-7 / 3.2e-7  (3.0e-7); 1.7e-6 / 1.8e-6 (8.7e-7) where the stem is louder than the mix and the result is the
                  small difference of two large terms
No kernel needed a change to meet them.
"""
import functools

import numpy as np
import pytest

from oracle import ensemble_oracle as E
from tests import ensemble_ref as R

pytestmark = pytest.mark.gpu

BAR = 5e-6
DELTA = 2e-5
# (N, K): seed whose K members, drawn in order from one generator, leave no ambiguous bin for "min" or for "max" (asserted below)
SHAPES = {(1024, 3): 1, (2047, 2): 0, (2048, 2): 1, (3000, 4): 2, (3071, 5): 3, (3072, 7): 12, (5121, 8): 25}
SHORT = {1: 0, 500: 0, 1023: 0}          # N < 1024 (K = 3): seeds with the same property
WAVE_EXACT = ("median_wave", "min_wave", "max_wave", "ensemble_wav")
WEIGHTS = ([1.0, 2.0, 0.5, 0.25], [1.0, -0.5, 3.0], [1.0, 1.0, 1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))
    yield e
    e.close()


def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(seed, n, k):
    m = R.members(seed, n, k)
    for x in m:
        x.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(seed, n, k, alg):
    r = R.ensemble(case(seed, n, k), alg)
    r.setflags(write=False)
    return r


def unambiguous(m):
    return R.ambiguous_bins(m, "min", DELTA) == 0 and R.ambiguous_bins(m, "max", DELTA) == 0


def spectral_ok(got, ref, n, what, peak=None):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e1 = R.scaled_err(got, ref, n, peak=peak)
    e2 = R.scaled_err(got, ref, n, peak="weighted") if peak is None else e1
    print(f"ENS {what} n={n} scaled_err {e1:.3e} weighted-peak {e2:.3e}")
    assert e1 <= BAR and e2 <= BAR, (what, e1, e2)


def wave_ok(eng, m, alg, weights=None):
    """wave-domain result of members m: bit for bit (avg_wave: against float64 within K + 1 float32 roundings of the terms' sum)"""
    got = eng.ensemble(m, alg, weights)
    if alg == "avg_wave":
        a = np.stack(m).astype(np.float64)
        wt = np.ones(len(m)) if weights is None else np.asarray(weights, np.float64)
        bound = (len(m) + 1) * 2.0 ** -24 * np.tensordot(np.abs(wt), np.abs(a), 1) / abs(wt.sum())
        assert got.dtype == np.float32 and (np.abs(got - R.ensemble(m, alg, weights)) <= bound).all(), alg
    else:
        want = E.ensemble(m, alg)
        assert want.dtype == np.float32 and np.array_equal(bits(got), bits(want)), alg
        assert alg == "median_wave" or np.array_equal(got, R.ensemble(m, alg))     # a selection is the same numbers in any precision


def means_apart(m):
    """ensemble_wav parity domain (include/asx.h): the engine sums |x| in float64, numpy in float32, so the two smallest channel means must
    differ by more than float32 summation can blur (1e-5 relative) -- or not at all"""
    for c in range(2):
        s = np.sort([np.abs(x[c].astype(np.float64)).mean() for x in m])
        if not (s[1] == s[0] or s[1] - s[0] > 1e-5 * s[1]):
            return False
    return True


# ---- spectral algorithms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", R.SPECTRAL)
@pytest.mark.parametrize("n,k", sorted(SHAPES))
def test_spectral(eng, n, k, alg):
    seed = SHAPES[(n, k)]
    m = case(seed, n, k)
    if alg in R.SELECTING:
        assert unambiguous(m), "the seed no longer gives members without near-ties: the comparison would not be defined"
    spectral_ok(eng.ensemble(m, alg), reference(seed, n, k, alg), n, alg)


@pytest.mark.parametrize("mult,alg,win", R.TIES)
def test_exact_ties(eng, mult, alg, win):
    m = R.tie_members(mult)
    got = eng.ensemble(m, alg)
    spectral_ok(got, R.ensemble(m, alg), R.TIE_N, f"tie{mult} {alg}")
    assert rel(got, R.roundtrip(win * m[0].astype(np.float64), got.shape[1])) <= 1e-3, f"{alg} of {mult} x w must be {win} x w"


@pytest.mark.parametrize("alg", R.SPECTRAL)
def test_same_member_twice(eng, alg):
    w = R.tie_members((1,))[0]
    got = eng.ensemble([w, w], alg)
    spectral_ok(got, R.ensemble([w, w], alg), R.TIE_N, f"[w, w] {alg}")
    assert rel(got, R.roundtrip(w, got.shape[1])) <= 1e-3


@pytest.mark.parametrize("wt", WEIGHTS)
def test_weights(eng, wt):
    m = case(5, 3000, len(wt))
    spectral_ok(eng.ensemble(m, "avg_fft", wt), R.ensemble(m, "avg_fft", wt), 3000, f"avg_fft weights {wt}")
    for n in (257, 4099):
        wave_ok(eng, case(6, n, len(wt)), "avg_wave", wt)
    # what Ensembler.ensemble does with unusable weights: equal weights
    for bad in ([1.0] * (len(wt) - 1), [0.0] * len(wt), [1.0, -1.0] + [0.0] * (len(wt) - 2), [np.inf] + [1.0] * (len(wt) - 1),
                [1e308, 1e308] + [1.0] * (len(wt) - 2)):
        with np.errstate(over="ignore"):                    # the sum of the last one overflows, which is the point
            assert np.array_equal(bits(eng.ensemble(m, "avg_wave", bad)), bits(eng.ensemble(m, "avg_wave")))


# ---- wave-domain algorithms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3, 8))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 4099))
def test_wave_bit_for_bit(eng, n, k):
    m = case(40 + k, n, k)
    assert means_apart(m)
    for alg in WAVE_EXACT + ("avg_wave",):
        wave_ok(eng, m, alg)


def test_wave_ties_and_signed_zeros(eng):
    w = case(7, 4099, 1)[0]
    for alg in ("min_wave", "max_wave", "median_wave"):
        wave_ok(eng, [w, -w, 2 * w], alg)
    assert np.array_equal(bits(eng.ensemble([w, -w, 2 * w], "min_wave")), bits(w))          # the first minimum
    assert np.array_equal(bits(eng.ensemble([w, 2 * w, -2 * w], "max_wave")), bits(2 * w))  # the first maximum
    assert np.array_equal(bits(eng.ensemble([w, -w], "ensemble_wav")), bits(w))             # equal means: the first member
    assert np.array_equal(bits(eng.ensemble([-w, w], "ensemble_wav")), bits(-w))
    # +0.0 against -0.0: |x| ties, and the sign bit of the winner is kept
    rng = np.random.default_rng(8)
    a, b = w.copy(), case(9, 4099, 1)[0].copy()
    z = rng.random(a.shape) < 0.3
    a[z] = np.where(rng.random(a.shape) < 0.5, 0.0, -0.0)[z].astype(np.float32)
    b[z] = -a[z]
    assert (np.signbit(a[z]) != np.signbit(b[z])).all() and np.signbit(a[z]).any() and not np.signbit(a[z]).all()
    for alg in ("min_wave", "max_wave", "ensemble_wav"):
        wave_ok(eng, [a, b], alg)
        wave_ok(eng, [b, a, b], alg)
    got = eng.ensemble([a, b], "min_wave")
    assert np.array_equal(bits(got)[z], bits(a)[z])
    # np.median leaves the order of equal keys open, so the sign of a zero median is compared by value only
    for m in ([a, b], [b, a, b]):
        got, want = eng.ensemble(m, "median_wave"), E.ensemble(m, "median_wave")
        assert np.array_equal(got, want) and np.array_equal(bits(got)[want != 0], bits(want)[want != 0])


def test_ensemble_wav_sums_in_float64(eng):
    """Outside the parity domain, documented beside asx_ensemble (include/asx.h): the engine's sums of |x| are float64, numpy's float32.
    Here numpy's two means round to the same float32 and the first member wins; the engine sees the true order and takes the second."""
    a = np.zeros((2, 4), np.float32)
    b = np.zeros((2, 4), np.float32)
    a[:, 0] = b[:, 0] = 1.0
    a[:, 1] = 2.0 ** -25
    assert np.array_equal(E.ensemble([a, b], "ensemble_wav"), a)
    assert np.array_equal(bits(eng.ensemble([a, b], "ensemble_wav")), bits(b))
    assert np.array_equal(bits(eng.ensemble([b, a], "ensemble_wav")), bits(b))
    assert np.array_equal(R.ensemble([a, b], "ensemble_wav"), b)


# ---- ragged members -----------------------------------------------------------------------------------------------------------------
RAGGED_SEED = 1


@pytest.mark.parametrize("alg", R.ALGORITHMS)
def test_ragged_members(eng, alg):
    """lengths (3000, 1000, 2049): Engine.ensemble pads with zeros, so the last frame of the second member is an exactly zero spectrum"""
    rng = np.random.default_rng(RAGGED_SEED)
    m = [(rng.standard_normal((2, n)) * 0.3).astype(np.float32) for n in (3000, 1000, 2049)]
    padded = [np.pad(x, ((0, 0), (0, 3000 - x.shape[1]))) for x in m]
    assert (R.stft(padded[1])[..., 2] == 0).all()
    if alg in R.SPECTRAL:
        assert alg not in R.SELECTING or unambiguous(padded)
        spectral_ok(eng.ensemble(m, alg), R.ensemble(padded, alg), 3000, f"ragged {alg}")
    else:
        assert means_apart(padded)
        got = eng.ensemble(m, alg)
        if alg == "avg_wave":
            bound = 4 * 2.0 ** -24 * np.abs(np.stack(padded).astype(np.float64)).sum(0) / 3
            assert (np.abs(got - R.ensemble(padded, alg)) <= bound).all()
        else:
            assert np.array_equal(bits(got), bits(E.ensemble(padded, alg)))


# ---- invert_stem --------------------------------------------------------------------------------------------------------------------
def stem_of(mix, seed, gain=0.5):
    noise = (np.random.default_rng(seed).standard_normal(mix.shape) * 0.3).astype(np.float32)
    return (np.float32(gain) * mix + np.float32(0.2) * noise).astype(np.float32)


def invert_ok(eng, mix, stem, what, peak=None):
    n = mix.shape[1]
    got = eng.invert_stem(mix, stem)
    assert got.shape == (1024 * (n // 1024), 2)
    spectral_ok(np.ascontiguousarray(got.T), R.invert_stem(mix, stem).T, n, f"invert_stem {what}", peak=peak)


@pytest.mark.parametrize("n", (1024, 2047, 3000, 5121))
def test_invert_stem(eng, n):
    mix = case(60, n, 1)[0]
    invert_ok(eng, mix, stem_of(mix, 61), "0.5 mix + 0.2 noise")


def test_invert_stem_edges(eng):
    n = 5121
    mix = case(60, n, 1)[0].copy()
    invert_ok(eng, mix, stem_of(mix, 61, gain=2.0), "stem louder than mix")
    # stem == mix: Y - |X| exp(j angle X) cancels to rounding (1e-16 of the mix in float64), so the error is taken over the mix's peak
    invert_ok(eng, mix, mix.copy(), "stem == mix", peak=float(np.abs(mix).max()))
    # two silent frames in the mix (samples 0 .. 2047): X = 0 there, its angle is 0, and the stem's bins lose |Y|
    mix[:, :2048] = 0.0
    assert (R.stft(mix)[..., :2] == 0).all() and (R.stft(mix)[..., 2:] != 0).any()
    stem = stem_of(mix, 61)
    invert_ok(eng, mix, stem, "silent mix frames, stem not silent")
    stem[:, :2048] = 0.0                                # and |X| = |Y| = 0
    invert_ok(eng, mix, stem, "silent mix and stem frames")
    invert_ok(eng, np.zeros_like(mix), stem, "all of the mix silent")


# ---- short inputs and limits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(SHORT))
def test_shorter_than_one_hop(eng, n):
    """N < 1024 is one frame: *_fft and the wave algorithms return [2, N]; uvr_* and invert_stem return hop * (T - 1) = 0 samples, like
    the reference, and launch nothing; the engine goes on answering"""
    m = case(SHORT[n], n, 3)
    assert unambiguous(m) and means_apart(m)
    for alg in R.ALGORITHMS:
        if alg.startswith("uvr_"):
            got = eng.ensemble(m, alg)
            assert got.shape == (2, 0) and got.dtype == np.float32 and R.ensemble(m, alg).shape == (2, 0)
        elif alg in R.SPECTRAL:
            spectral_ok(eng.ensemble(m, alg), reference(SHORT[n], n, 3, alg), n, f"short {alg}")
        else:
            wave_ok(eng, m, alg)
    got = eng.invert_stem(m[0], m[1])
    assert got.shape == (0, 2) and got.dtype == np.float32 and R.invert_stem(m[0], m[1]).shape == (0, 2)
    big = case(SHAPES[(3000, 4)], 3000, 4)
    for alg in ("uvr_min_spec", "median_fft"):
        spectral_ok(eng.ensemble(big, alg), reference(SHAPES[(3000, 4)], 3000, 4, alg), 3000, f"after short {alg}")
    invert_ok(eng, big[0], big[1], "after short")


def test_member_count_limits(eng):
    import audio_separator_amd as A
    m = case(70, 1500, 9)
    for alg in ("avg_wave", "median_fft", "ensemble_wav", "uvr_max_spec"):
        with pytest.raises(A.AsxError, match="9 inputs"):
            eng.ensemble(m, alg)
        got = eng.ensemble(m[:1], alg)                       # one member: returned as it is
        assert np.array_equal(bits(got), bits(m[0]))
    empty = [np.zeros((2, 0), np.float32)] * 2
    with pytest.raises(A.AsxError):
        eng.ensemble(empty, "avg_fft")
    with pytest.raises(A.AsxError):
        eng.invert_stem(empty[0], empty[1])
    with pytest.raises(ValueError):
        eng.ensemble(m[:2], "nope")
    m8 = case(SHAPES[(5121, 8)], 5121, 8)
    spectral_ok(eng.ensemble(m8, "median_fft"), reference(SHAPES[(5121, 8)], 5121, 8, "median_fft"), 5121, "after refusals median_fft")
