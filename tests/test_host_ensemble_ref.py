"""The float64 references of tests/test_gpu_ensemble_kernels.py (tests/ensemble_ref.py), checked without a GPU: against the golden
vectors the reference's own Ensembler / invert_stem wrote, against the project's CPU oracle fed float64 (two independent statements of
one operation), the mutants that show the GPU test's bars bite at exact ties, and what a float32 implementation needs of the bar.

Measured here (seeds 100-102, N in SIZES, K in (2, 3, 8)), the float32 oracle against ensemble_ref, the larger of scaled_err over the
plain and over the weighted peak: 2.0e-7 avg_fft, 2.2e-7 median_fft, 2.4e-7 min_fft, 2.2e-7 max_fft, 2.2e-7 uvr_max_spec, 2.4e-7
uvr_min_spec, 1.9e-7 invert_stem -- the GPU bar of 5e-6 is about 20x that.  The float64 oracle agrees with ensemble_ref to 8.2e-16 in scaled_err; in the plain max-error-over-peak metric the same
pairs differ by up to 9e-12 at N = 1024 k - 1, which is the ill-conditioned last hop and the reason the metric weighs by the window sum.
"""
import os

import numpy as np
import pytest

from oracle import ensemble_oracle as E
from tests import ensemble_ref as R

SIZES = (1024, 1500, 2047, 2048, 3000, 3071, 4095, 5121)
KS = (2, 3, 8)
GPU_BAR = 5e-6          # tests/test_gpu_ensemble_kernels.py


def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "ensemble_small.npz"))


def test_algorithm_names():
    assert R.ALGORITHMS == E.ALGORITHMS and set(R.SPECTRAL) | {"avg_wave", "median_wave", "min_wave", "max_wave", "ensemble_wav"} == set(E.ALGORITHMS)


def test_golden_every_key(g):
    w = [g["waves"][k] for k in range(4)]
    seen = {"waves"}
    for alg in R.ALGORITHMS:
        for k in (4, 3):
            assert rel(R.ensemble(w[:k], alg), g[f"{alg}_k{k}"]) <= 1e-6, (alg, k)
            seen.add(f"{alg}_k{k}")
    for alg in ("avg_wave", "avg_fft"):
        assert rel(R.ensemble(w, alg, [1.0, 2.0, 0.5, 0.25]), g[f"{alg}_w"]) <= 1e-6, alg
        seen.add(f"{alg}_w")
    assert rel(R.invert_stem(w[0], w[1]), g["invert"]) <= 1e-6
    seen.add("invert")
    assert seen == set(g.files)


@pytest.mark.parametrize("n", SIZES + (1, 500, 1023))
def test_against_float64_oracle(n):
    """Wave algorithms: the same numbers.  Spectral: 1e-12 in scaled_err (the two differ in float64 rounding alone, and the last hop of
    a length-N result multiplies that by up to sqrt(2 / 5e-12), module docstring)."""
    for K in KS:
        m = [x.astype(np.float64) for x in R.members(100, n, K)]
        for alg in R.ALGORITHMS:
            a, b = R.ensemble(m, alg), E.ensemble(m, alg)
            assert a.shape == b.shape and a.dtype == np.float64
            if a.size:
                assert (R.scaled_err(a, b, n) if alg in R.SPECTRAL else rel(a, b)) <= 1e-12, (alg, K)
        wt = np.linspace(-0.5, 2.0, K)
        for alg in ("avg_wave", "avg_fft"):
            a, b = R.ensemble(m, alg, wt), E.ensemble(m, alg, wt)
            assert (R.scaled_err(a, b, n) if alg == "avg_fft" else rel(a, b)) <= 1e-12, (alg, K)
        a, b = R.invert_stem(m[0], m[1]), E.invert_stem(m[0], m[1])
        assert a.shape == b.shape == (1024 * (n // 1024), 2)
        if a.size:
            assert R.scaled_err(a.T, b.T, n) <= 1e-12


def test_shapes_and_window_sum():
    m = R.members(0, 1500, 3)
    assert R.ensemble(m, "uvr_min_spec").shape == (2, 1024) and R.ensemble(m, "min_fft").shape == (2, 1500)
    assert R.ensemble(R.members(0, 1023, 2), "uvr_max_spec").shape == (2, 0)
    assert R.invert_stem(*R.members(0, 500, 2)).shape == (0, 2)
    assert np.array_equal(R.ensemble(m[:1], "median_fft"), m[0])
    s = R.wss(3000, 3000)                                   # three frames; two overlap in the interior: sin^4 + cos^4, in [0.5, 1]
    th = np.pi * np.arange(1024) / 2048
    assert s.shape == (3000,) and np.allclose(s[:2048], np.tile(np.sin(th) ** 4 + np.cos(th) ** 4, 2), atol=1e-12, rtol=0)
    assert s[:2048].min() == pytest.approx(0.5) and s[:2048].max() == pytest.approx(1.0)
    w = R.window()
    assert np.allclose(s[2048:], w[1024: 1024 + 952] ** 2, atol=1e-15, rtol=0)     # the last hop: the last frame alone
    assert R.wss(2047, 2047)[-1] == pytest.approx(w[2046] ** 2) and 8e-11 < w[2046] ** 2 < 9e-11    # and w[2047]^2 = 5.5e-12 one further
    assert R.scaled_err(np.ones((2, 2047)), np.ones((2, 2047)) * (1 + 1e-3), 2047) == pytest.approx(1e-3 / (1 + 1e-3))


def test_ambiguous_bins_counts():
    w = R.members(3, 2048, 1)[0]
    assert R.ambiguous_bins([w, w * np.float32(1 + 2.0 ** -20)], "min", 2e-5) > 2000          # gaps of 1e-6 |X|
    assert R.ambiguous_bins([w, 2 * w], "min", 2e-5) == R.ambiguous_bins([w, 2 * w], "max", 2e-5)
    assert R.ambiguous_bins([w, 2 * w], "max", 1e-12) == 0
    assert R.ambiguous_bins([w, -w, 2 * w], "min", 2e-5) == 2 * 1025 * 3 and R.ambiguous_bins([w, -w, 2 * w], "max", 2e-5) < 50


@pytest.mark.parametrize("mutant,mult", [("min_fft_last", (1, -1, 2)), ("uvr_max_spec_first", (1, 2, -2)), ("median_fft_mag", (1, -1, 2))])
def test_mutants_exceed_the_gpu_bar_at_ties(mutant, mult):
    """a kernel with the wrong tie rule (or a median of magnitudes) is at least 100 x the GPU bar away on the tie inputs"""
    alg = next(a for a in R.SPECTRAL if mutant.startswith(a))
    assert (mult, alg) in [(t[0], t[1]) for t in R.TIES]
    m = R.tie_members(mult)
    err = R.scaled_err(R.ensemble(m, alg, mutant=mutant), R.ensemble(m, alg), R.TIE_N)
    print(f"{mutant}: scaled_err {err:.3e}")
    assert err >= 100 * GPU_BAR
    r = R.members(11, 3000, 3)                              # and they are the right rule wherever nothing ties
    if mutant != "median_fft_mag":
        assert R.scaled_err(R.ensemble(r, alg, mutant=mutant), R.ensemble(r, alg), 3000) <= 1e-12


def test_tie_winners_in_the_reference():
    for mult, alg, win in R.TIES:
        m = R.tie_members(mult)
        w = m[0].astype(np.float64)
        got = R.ensemble(m, alg)
        assert R.scaled_err(got, R.roundtrip(win * w, got.shape[-1]), R.TIE_N) <= 1e-12, (mult, alg)


@pytest.mark.parametrize("n", SIZES)
def test_float32_oracle_needs_a_twentieth_of_the_gpu_bar(n):
    worst = {}
    for K in KS:
        for seed in (100, 101, 102):
            m = R.members(seed, n, K)
            for alg in R.SPECTRAL:
                got, ref = E.ensemble(m, alg), R.ensemble(m, alg)
                worst[alg] = max(worst.get(alg, 0.0), R.scaled_err(got, ref, n), R.scaled_err(got, ref, n, peak="weighted"))
            worst["invert_stem"] = max(worst.get("invert_stem", 0.0), R.scaled_err(E.invert_stem(m[0], m[1]).T, R.invert_stem(m[0], m[1]).T, n))
    print(n, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 5e-7, worst
