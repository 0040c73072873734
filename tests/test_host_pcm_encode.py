"""What the writer edge of use_soundfile=True decides on the host, without a device: the refusals of asx_pcm_encode*, asx_flac_plan_pcm and
asx_flac_encode_pcm* (every argument is judged before the engine is touched, the engine last, so a NULL engine with otherwise good arguments
reaches each of them), the plan of the int32 FLAC form against its formula, and audio_io.write_wav_body against audio_io.write_wav."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
from audio_separator_amd import audio_io
from audio_separator_amd import engine as E
from tests.flac_wide_cases import worst_frame


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return E.load_library()


def _err(lib):
    return (lib.asx_last_error() or b"").decode()


P = 0x10000          # a non-null, 16-byte aligned address that no refusal dereferences


def test_pcm_encode_dev_refusals(lib):
    f = lib.asx_pcm_encode_dev
    good = dict(e=None, stem=P, n=100, layout=1, mx=0.9, mn=0.0, has_min=1, fmt=24, out=P, peak=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["e"], a["stem"], a["n"], a["layout"], a["mx"], a["mn"], a["has_min"], a["fmt"], a["out"], a["peak"], a["stream"])
    for kw, text in (({"stem": None}, "null stem or output"), ({"out": None}, "null stem or output"), ({"n": 0}, "n_samples = 0"),
                     ({"n": -5}, "n_samples = -5"), ({"layout": 2}, "layout 2"), ({"layout": -1}, "layout -1"), ({"fmt": 8}, "sample format 8"),
                     ({"fmt": 64}, "sample format 64"), ({"fmt": 0x140}, "sample format 320"), ({"out": P + 4}, "16-byte aligned"),
                     ({"stem": P + 2}, "4-byte"), ({}, "null engine")):
        assert call(**kw) != 0, kw
        assert "asx_pcm_encode_dev" in _err(lib) and text in _err(lib), (kw, _err(lib))
    for fmt in (16, 24, 32, 0x120, 0x410, 0x418):                 # every known format passes the format check
        assert call(fmt=fmt) != 0 and "null engine" in _err(lib)
    for layout in (0, 1):
        assert call(layout=layout) != 0 and "null engine" in _err(lib)


def test_pcm_encode_host_refusals(lib):
    f = lib.asx_pcm_encode
    x = np.zeros((8, 2), np.float32)
    out = np.zeros(64, np.uint8)
    xp, op = x.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data

    def call(stem=xp, n=8, layout=1, fmt=16, o=op):
        return f(None, stem, n, layout, 0.9, 0.0, 0, fmt, o, None)
    for kw, text in (({"stem": None}, "null stem or output"), ({"o": None}, "null stem or output"), ({"n": 0}, "n_samples = 0"),
                     ({"layout": 7}, "layout 7"), ({"fmt": 20}, "sample format 20"), ({}, "null engine")):
        assert call(**kw) != 0, kw
        assert "asx_pcm_encode:" in _err(lib) and text in _err(lib), (kw, _err(lib))


def test_flac_encode_pcm_refusals(lib):
    total = C.c_int64()
    dev = lambda **kw: lib.asx_flac_encode_pcm_dev(kw.get("e"), kw.get("pcm", P), kw.get("n", 100), kw.get("rate", 44100), kw.get("bits", 24),  # noqa: E731
                                                   kw.get("block", 4096), kw.get("out", P), kw.get("cap", 1 << 20), kw.get("sizes", P),
                                                   C.byref(total), None)
    for kw, text in (({"bits": 20}, "20 bits per sample"), ({"bits": 32}, "32 bits per sample"), ({"block": 15}, "block size 15"),
                     ({"block": 4609}, "block size 4609"), ({"n": 0}, "no samples"), ({"rate": 0}, "sample rate 0"),
                     ({"rate": 1 << 20}, "sample rate"), ({"pcm": None}, "null argument"), ({"out": None}, "null argument"),
                     ({"sizes": None}, "null argument"), ({}, "null argument")):
        assert dev(**kw) != 0, kw
        assert "asx_flac_encode_pcm_dev" in _err(lib) and text in _err(lib), (kw, _err(lib))
    pcm = np.zeros((100, 2), np.int32)
    out = np.zeros(1 << 16, np.uint8)
    sizes = np.zeros(1, np.int32)
    host = lambda **kw: lib.asx_flac_encode_pcm(None, kw.get("pcm", pcm.ctypes.data_as(C.POINTER(C.c_int32))), kw.get("n", 100), kw.get("rate", 44100),  # noqa: E731
                                                kw.get("bits", 16), kw.get("block", 4096), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size,
                                                sizes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(total))
    for kw, text in (({"bits": 8}, "8 bits per sample"), ({"block": 5000}, "block size 5000"), ({"n": -1}, "no samples"),
                     ({"rate": -3}, "sample rate -3"), ({"pcm": None}, "null argument"), ({}, "null argument")):
        assert host(**kw) != 0, kw
        assert "asx_flac_encode_pcm:" in _err(lib) and text in _err(lib), (kw, _err(lib))


@pytest.mark.parametrize("bits", [16, 24])
def test_flac_plan_pcm_follows_its_formula(lib, bits):
    for n, block in ((1, 4096), (4096, 4096), (4097, 4096), (3 * 4096 + 17, 4096), (10_584_000, 4096), (5000, 16), (5000, 1000), (9221, 4608)):
        plan = E.Engine.flac_plan_pcm(n, 2, bits, block)
        nb = -(-n // block)
        last = n - (nb - 1) * block
        stride = -(-worst_frame(block, bits) // 16) * 16
        assert plan == {"n_blocks": nb, "frame_stride": stride, "max_bytes": (nb - 1) * worst_frame(block, bits) + worst_frame(last, bits),
                        "scratch_bytes": nb * stride + (nb + 1) * 8}, (n, block)
    # the int16 form's plan is what it was: both of its streams budget 17 bits per sample
    assert E.Engine.flac_plan(4097, 2, 24, 4096)["frame_stride"] == E.Engine.flac_plan_pcm(4097, 2, 16, 4096)["frame_stride"] == -(-worst_frame(4096, 16) // 16) * 16


def test_flac_plan_pcm_refusals(lib):
    for args, text in (((100, 1, 24, 4096), "1 channels"), ((100, 2, 20, 4096), "20 bits per sample"), ((100, 2, 24, 8), "block size 8"),
                       ((100, 2, 24, 4609), "block size 4609"), ((0, 2, 24, 4096), "no samples")):
        with pytest.raises(E.AsxError, match=text):
            E.Engine.flac_plan_pcm(*args)
    assert lib.asx_flac_plan_pcm(100, 2, 24, 4096, None, None, None, None) == 0      # any out pointer may be NULL


def _body(x, subtype):
    """the data chunk numpy makes of float32 [n, 2] by audio_io.write_wav's rule"""
    if subtype == "FLOAT":
        return x.astype("<f4").tobytes()
    bits = int(subtype[4:])
    full = float(2 ** (bits - 1) - 1)
    v = np.clip(np.rint(x.astype(np.float64) * full), -full - 1, full).astype(np.int64)
    if bits == 24:
        return (v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    return v.astype("<i2" if bits == 16 else "<i4").tobytes()


@pytest.mark.parametrize("subtype", ["PCM_16", "PCM_24", "PCM_32", "FLOAT"])
def test_write_wav_body_equals_write_wav(tmp_path, subtype):
    rng = np.random.default_rng(3)
    for n in (1, 5, 1021):
        x = rng.uniform(-1.2, 1.2, (n, 2)).astype(np.float32)
        x[0] = (1.0, -1.0)
        a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
        audio_io.write_wav(a, x, 48000, subtype)
        body = _body(x, subtype)
        audio_io.write_wav_body(b, np.frombuffer(body, np.uint8), 48000, subtype, n)
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read()
        assert audio_io.wav_info(b)["frames"] == n and audio_io.info(b)["subtype"] == subtype
    with pytest.raises(audio_io.AudioIOError, match="frames"):
        audio_io.write_wav_body(b, body, 48000, subtype, n + 1)
    with pytest.raises(audio_io.AudioIOError, match="subtype"):
        audio_io.write_wav_body(b, body, 48000, "DOUBLE", n)
