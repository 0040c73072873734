"""csrc/resample_plan.h -- the filter design, the length rule, the device table and the float64 evaluation of the rational polyphase
converter (asx_resample_rational) -- compiled with g++ into tests/host/resample_plan_host.cpp, once plainly and once with
-fsanitize=address,undefined, against an independent numpy restatement of the design (scipy.signal.kaiserord, np.kaiser, np.sinc) and
against analytic sines; then the same plan numbers through libasx.so.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "resample_plan_host.cpp")

PAIRS = [(48000, 44100), (96000, 44100), (88200, 44100), (32000, 44100), (22050, 44100), (8000, 44100), (192000, 44100), (44100, 48000)]
REFUSED = [(44056, 44100), (44100, 44100)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resample") / f"resample_plan_host_{request.param}")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", out, SRC], check=True)
    return out


def run(exe, *args, binary=None):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True)
    if binary is None:
        return r.returncode, r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0, (args, r.returncode, r.stderr.decode())
    return np.frombuffer(r.stdout, dtype=binary)


def design(sr_in, sr_out):
    """The design of the issue, restated with scipy / numpy: (L, M, N, half, T, taps float64 [2 half + 1])."""
    from scipy.signal import kaiserord
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    G = max(L, M)
    fpass, fstop = 0.913 / G, 1.0 / G
    N, beta = kaiserord(125.0, fstop - fpass)
    assert beta == 0.1102 * (125.0 - 8.7)
    half = -(-(N - 1) // (2 * L)) * L                      # ceil((N - 1) / 2 / L) * L
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = 0.5 * (fpass + fstop)
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
    return L, M, int(N), half, 2 * half // L + 1, h * (L / h.sum())


def plan_line(exe, sr_in, sr_out, *n_in):
    rc, out, err = run(exe, "plan", sr_in, sr_out, *n_in)
    assert rc == 0, (out, err)
    lines = out.splitlines()
    assert lines[0].startswith("plan ")
    return [int(v) for v in lines[0].split()[1:]], [tuple(int(v) for v in ln.split()[1:]) for ln in lines[1:]]


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_plan_and_taps_match_the_numpy_restatement(exe, sr_in, sr_out):
    L, M, N, half, T, h = design(sr_in, sr_out)
    (gL, gM, gN, ghalf, gT, J, K, span, lds), _ = plan_line(exe, sr_in, sr_out)
    assert (gL, gM, gN, ghalf, gT) == (L, M, N, half, T)
    taps = run(exe, "taps", sr_in, sr_out, binary=np.float64)
    assert taps.shape == h.shape
    print(f"{sr_in}->{sr_out}: L {L} M {M} N {N} half {half} T {T}; max |tap - numpy| = {np.abs(taps - h).max():.3e}")
    assert np.abs(taps - h).max() <= 1e-12
    assert abs(taps.sum() - L) <= 1e-9
    # the tile: whole periods, inside the LDS budget the kernel is launched with
    assert J % L == 0 and K in (1, 2, 4, 8) and span == J // L * K * M + T
    assert span + (L * T if lds else 0) <= 16384


def test_taps_per_output_of_the_common_pairs(exe):
    """The figures the kernel's notes quote."""
    want = {(48000, 44100): (147, 160, 205), (96000, 44100): (147, 320, 409), (32000, 44100): (441, 320, 189),
            (22050, 44100): (2, 1, 189), (88200, 44100): (1, 2, 377)}
    for (a, b), (L, M, T) in want.items():
        (gL, gM, _, _, gT, *_), _ = plan_line(exe, a, b)
        assert (gL, gM, gT) == (L, M, T)


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_device_table_is_the_taps_by_output_residue(exe, sr_in, sr_out):
    L, M, _, half, T, h = design(sr_in, sr_out)
    tab = run(exe, "table", sr_in, sr_out, binary=np.float32).reshape(T, L)
    P = half // L
    r = np.arange(L)
    n = (r * M) % L + (np.arange(T)[:, None] - P) * L
    want = np.where(np.abs(n) <= half, h[np.clip(n + half, 0, 2 * half)], 0.0).astype(np.float32)
    # float32 roundings of taps that agree to 1e-12 may differ by one unit in the last place
    assert np.abs(tab - want).max() <= np.spacing(np.float32(np.abs(want).max()))
    assert (tab != want).mean() < 1e-3
    # ... and the sum the kernel forms over that table is the definition
    rc, out, err = run(exe, "layout", sr_in, sr_out, 700)
    assert rc == 0, err
    assert float(out) <= 1e-12


def sine_error(exe, sr_in, sr_out, f, phi, n_in):
    L, M, _, half, T, _ = design(sr_in, sr_out)
    n_out = -(-n_in * L // M)
    # The filter reaches T inputs, which are T * L / M outputs when L > M: the margin the issue states, T * max(1, M / L) + 2, is widened to
    # the filter's whole length in outputs for upsampling (it is unchanged for M >= L), so that no compared output sees the zero history.
    edge = int(math.ceil(T * max(1.0, M / L, L / M))) + 2
    assert n_out > 2 * edge + 200
    y = run(exe, "sine", sr_in, sr_out, repr(f), repr(phi), n_in, edge, n_out - edge, binary=np.float64)
    m = np.arange(edge, n_out - edge, dtype=np.float64)
    return y, np.sin(2.0 * np.pi * f * m / sr_out + phi)


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_passband_sines_within_the_kaiser_ripple(exe, sr_in, sr_out):
    """evaluate() on unit sines in the pass band: 10^(-125 / 20) = 5.6e-7 is the design's ripple, 6e-7 the bound."""
    nyq = min(sr_in, sr_out) / 2.0
    L, M, _, _, T, _ = design(sr_in, sr_out)
    n_in = int(math.ceil((2 * T * max(1.0, M / L, L / M) + 400) * M / L)) + 8
    worst = 0.0
    for f, phi in ((100.0, 0.3), (1000.0, 1.1), (0.5 * nyq, 0.0), (0.9 * nyq, 2.0)):
        y, want = sine_error(exe, sr_in, sr_out, f, phi, n_in)
        err = float(np.abs(y - want).max())
        print(f"{sr_in}->{sr_out} {f:9.1f} Hz: max error {err:.3e} over {y.size} outputs")
        worst = max(worst, err)
    assert worst <= 6e-7


@pytest.mark.parametrize("sr_in,sr_out", [p for p in PAIRS if p[0] > p[1]])
def test_stopband_sines_below_minus_120_db(exe, sr_in, sr_out):
    nyq = sr_out / 2.0
    L, M, _, _, T, _ = design(sr_in, sr_out)
    n_in = int(math.ceil((2 * T * M / L + 400) * M / L)) + 8
    for f, phi in ((nyq + 50.0, 0.4), (1.05 * nyq, 1.3)):
        y, _ = sine_error(exe, sr_in, sr_out, f, phi, n_in)
        db = 20.0 * math.log10(max(float(np.abs(y).max()), 1e-300))
        print(f"{sr_in}->{sr_out} {f:9.1f} Hz: {db:.1f} dB")
        assert db <= -120.0


def test_output_lengths(exe):
    ns = [1, 2, 159, 160, 161, 10 ** 7 + 1]
    for sr_in, sr_out in PAIRS:
        L, M = design(sr_in, sr_out)[:2]
        _, got = plan_line(exe, sr_in, sr_out, *ns)
        assert got == [(n, -(-n * L // M)) for n in ns]
    _, got = plan_line(exe, 48000, 44100, *ns)
    assert [o for _, o in got] == [1, 2, 147, 147, 148, 9187501]


@pytest.mark.parametrize("sr_in,sr_out", REFUSED)
def test_refusals(exe, sr_in, sr_out):
    rc, out, _ = run(exe, "plan", sr_in, sr_out)
    assert rc == 3 and out.startswith("error ")
    assert ("equal" in out) if sr_in == sr_out else ("2^20" in out)


# ---- through the library -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from audio_separator_amd import engine as E
    entry.build()
    return E.load_library(), E


def test_library_plan_matches(lib):
    _, E = lib
    for sr_in, sr_out in PAIRS:
        L, M, _, _, T, _ = design(sr_in, sr_out)
        for n in (1, 2, 159, 160, 161, 10 ** 7 + 1):
            assert E.Engine.resample_rational_plan(sr_in, sr_out, n) == (-(-n * L // M), L, M, T)


def test_library_refusals_carry_a_message(lib):
    l, E = lib
    for sr_in, sr_out in REFUSED:
        with pytest.raises(E.AsxError, match="equal" if sr_in == sr_out else "2\\^20"):
            E.Engine.resample_rational_plan(sr_in, sr_out, 100)
    with pytest.raises(E.AsxError, match="n_in"):
        E.Engine.resample_rational_plan(48000, 44100, 0)
    # the optional outputs may be NULL
    assert l.asx_resample_rational_plan(48000, 44100, 0, None, None, None, None) == 0


def test_null_engine_is_an_error_not_a_crash(lib):
    l, _ = lib
    x = (C.c_float * 8)()
    assert l.asx_resample_rational_dev(None, C.cast(x, C.c_void_p), 1, 8, 48000, 44100, C.cast(x, C.c_void_p), 8, None) != 0
    assert b"asx_resample_rational_dev" in l.asx_last_error()
    assert l.asx_resample_rational(None, x, 1, 8, 48000, 44100, x, 8) != 0
