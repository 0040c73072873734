"""asx_pcm_encode / asx_pcm_encode_dev (csrc/kernels_pcm_encode.h) against numpy, byte for byte: spec_utils.normalize in float32, then
clip(rint(float64(x) * (2^(b-1) - 1)), -2^(b-1), 2^(b-1) - 1) for the integer formats (audio_io.write_wav's rule), the value itself for float32.
Every operation of the reference is a single correctly rounded IEEE operation, so there is no tolerance: the bytes are equal or the kernel is
wrong.  Sizes: a lane takes four frames, so 1, 2, 3 and 5 are the tail alone and a group plus a tail, 255 / 256 / 257 and 1021 / 4099 end
inside and on a group and a workgroup (1024 frames), 70001 takes many workgroups; planar stems with n % 4 != 0 take the scalar loads."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 255, 256, 257, 1021, 4099, 70001)
FORMATS = ("PCM_16", "PCM_24", "PCM_32", "FLOAT", "S16_IN_32", "S24_IN_32")
BITS = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32, "S16_IN_32": 16, "S24_IN_32": 24}
# (peak of the data, max_peak, min_peak): scaled down, amplified, untouched, no lower threshold
NORMS = ((1.7, 0.9, 0.0), (0.2, 0.9, 0.5), (0.7, 0.9, 0.5), (0.2, 0.9, None))


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(), device=0)
    yield e
    e.close()


def normalize(x, max_peak, min_peak):
    """spec_utils.normalize in float32: one division, one product per sample"""
    maxv = np.float32(np.abs(x).max())
    if maxv > np.float32(max_peak):
        return x * (np.float32(max_peak) / maxv)
    if min_peak is not None and maxv < np.float32(min_peak):
        return x * (np.float32(min_peak) / maxv)
    return x


def encode(x, fmt):
    """normalised float32 [n, 2] -> the array Engine.pcm_encode returns"""
    if fmt == "FLOAT":
        return x.astype("<f4")
    bits = BITS[fmt]
    full = float(2 ** (bits - 1) - 1)
    v = np.clip(np.rint(x.astype(np.float64) * full), -full - 1, full).astype(np.int64)
    if fmt == "PCM_16":
        return v.astype("<i2")
    if fmt == "PCM_24":
        return np.ascontiguousarray(v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1, 6)
    return v.astype("<i4")


@pytest.fixture(scope="module")
def stems():
    """float32 [n, 2] per (size, normalisation), made once"""
    rng = np.random.default_rng(11)
    out = {}
    for n in SIZES:
        for j, (peak, _, _) in enumerate(NORMS):
            x = rng.uniform(-peak, peak, (n, 2)).astype(np.float32)
            x[rng.integers(0, n), rng.integers(0, 2)] = peak            # the peak itself, on either channel
            out[n, j] = x
    return out


def _check(eng, x, fmt, layout, max_peak, min_peak):
    want_x = normalize(x, max_peak, min_peak)
    arg = x if layout == "rows" else np.ascontiguousarray(x.T)
    got, peak = eng.pcm_encode(arg, fmt, max_peak, min_peak, layout=layout)
    want = encode(want_x, fmt)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (fmt, layout, x.shape, max_peak, min_peak, np.argwhere(got != want)[:4])
    assert np.float32(peak) == np.abs(want_x).max() and isinstance(peak, float)


@pytest.mark.parametrize("layout", ["rows", "planar"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_bytes_equal_numpy(eng, stems, fmt, layout):
    for n in SIZES:
        for j, (_, max_peak, min_peak) in enumerate(NORMS):
            _check(eng, stems[n, j], fmt, layout, max_peak, min_peak)


@pytest.mark.parametrize("layout", ["rows", "planar"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_full_scale_clipping_and_ties(eng, fmt, layout):
    # +-1.0 with max_peak 1.0: untouched, the largest code and its negative, nothing clips
    x = np.zeros((257, 2), np.float32)
    x[3], x[200] = (1.0, -1.0), (-1.0, 1.0)
    _check(eng, x, fmt, layout, 1.0, 0.0)
    if fmt != "FLOAT":
        top = 2 ** (BITS[fmt] - 1) - 1
        got, _ = eng.pcm_encode(x if layout == "rows" else np.ascontiguousarray(x.T), fmt, 1.0, 0.0, layout=layout)
        v = got if fmt != "PCM_24" else None
        if v is not None:
            assert v[3].tolist() == [top, -top] and v[200].tolist() == [-top, top]
    # a threshold of 1.5 leaves values up to 1.4 in place: both ends clip
    rng = np.random.default_rng(5)
    y = rng.uniform(-1.4, 1.4, (1021, 2)).astype(np.float32)
    y[0], y[1] = (1.4, -1.4), (-1.0000001, 1.0000001)
    _check(eng, y, fmt, layout, 1.5, 0.0)
    if fmt not in ("FLOAT", "PCM_24"):
        got, _ = eng.pcm_encode(y if layout == "rows" else np.ascontiguousarray(y.T), fmt, 1.5, 0.0, layout=layout)
        top = 2 ** (BITS[fmt] - 1) - 1
        assert got.max() == top and got.min() == -top - 1
    # rounding ties: +-0.5 times an odd full scale is k + 0.5 exactly (to even), and float32((k + 0.5) / full) lands on either side of a tie
    full = float(2 ** (BITS.get(fmt, 16) - 1) - 1)
    k = np.concatenate([np.arange(-40, 40), rng.integers(-int(full), int(full), 900)]).astype(np.float64)
    t = ((k + 0.5) / full).astype(np.float32)
    z = np.stack([t, -t], 1)
    z[:4] = [(0.5, -0.5), (-0.5, 0.5), (0.25, 0.75), (-0.25, -0.75)]
    assert np.abs(z).max() <= 1.0
    _check(eng, z, fmt, layout, 1.0, None)


def test_silent_stem_has_peak_zero(eng):
    for fmt in FORMATS:
        got, peak = eng.pcm_encode(np.zeros((300, 2), np.float32), fmt, 0.9, 0.0)
        assert peak == 0.0 and not got.any()


def test_device_call_leaves_the_stem_alone_and_takes_unaligned_rows(eng, stems):
    import torch
    for layout in ("rows", "planar"):
        for n in (5, 257, 4099):
            x = stems[n, 0]
            arg = x if layout == "rows" else np.ascontiguousarray(x.T)
            buf = torch.zeros(2 * n + 3, dtype=torch.float32, device="cuda")
            for off in (0, 1, 3):                                       # 16-byte aligned, and 4- / 12-byte offsets: the scalar loads
                stem = buf[off:off + 2 * n]
                stem.copy_(torch.from_numpy(arg.reshape(-1)))
                before = stem.clone()
                out = torch.zeros(6 * n + 16, dtype=torch.uint8, device="cuda")
                peak = eng.pcm_encode_dev(stem.data_ptr(), n, layout, 0.9, 0.0, "PCM_24", out.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(stem, before)
                want = encode(normalize(x, 0.9, 0.0), "PCM_24")
                assert out[:6 * n].cpu().numpy().tobytes() == want.tobytes(), (layout, n, off)
                assert not out[6 * n:].any()                            # nothing behind the body
                assert np.float32(peak) == np.abs(normalize(x, 0.9, 0.0)).max()


def test_device_call_refuses_bad_arguments(eng):
    import audio_separator_amd as A
    import torch
    stem = torch.zeros((100, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros(800, dtype=torch.uint8, device="cuda")
    with pytest.raises(A.AsxError, match="n_samples"):
        eng.pcm_encode_dev(stem.data_ptr(), 0, "rows", 0.9, 0.0, "PCM_16", out.data_ptr())
    with pytest.raises(A.AsxError, match="null stem or output"):
        eng.pcm_encode_dev(stem.data_ptr(), 100, "rows", 0.9, 0.0, "PCM_16", 0)
    with pytest.raises(A.AsxError, match="16-byte aligned"):
        eng.pcm_encode_dev(stem.data_ptr(), 100, "rows", 0.9, 0.0, "PCM_16", out.data_ptr() + 4)
    with pytest.raises(ValueError, match="subtype"):
        eng.pcm_encode_dev(stem.data_ptr(), 100, "rows", 0.9, 0.0, "DOUBLE", out.data_ptr())


def test_silent_device_stem_writes_no_file(tmp_path, monkeypatch):
    """a stem of zeros that is still in HBM: the writer warns and leaves no file, and its entry is released"""
    import torch
    from audio_separator_amd import audio_io
    from tests import separate_cases as SC
    real = audio_io._optional
    monkeypatch.setattr(audio_io, "_optional", lambda name: None if name == "soundfile" else real(name))
    _, cls, common, arch, _, _ = SC.cases("mdx", str(tmp_path))[0]
    inst = SC.plugin_class(cls)(common_config=dict(common, use_soundfile=True), arch_config=arch)
    inst.input_subtype, inst.input_bit_depth = "PCM_24", 24
    for name in ("silent.wav", "silent.flac"):
        arr = inst._host_stem(torch.zeros((1000, 2), dtype=torch.float32, device="cuda"))
        inst.last_write_path = None
        inst.write_audio_soundfile(name, arr)
        assert inst._dev_stems == {} and inst.last_write_path is None
        assert not (tmp_path / "out" / name).exists() and not (tmp_path / name).exists()
    inst.clear_gpu_cache()
