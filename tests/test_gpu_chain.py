"""workflow.ChainSeparator on the device: the files of the literal flow (``first.separate`` -> the stem's file -> ``then.separate``),
byte for byte, with the stem handed over in HBM -- every plugin family once as the first and once as the second stage, the default WAV
and FLAC writers, ``use_soundfile``, a 48 kHz and a FLAC input, ``separate_many`` -- the float hand-off against the flow through a
32-bit float file, and a mix-down against the writer applied to tests/mixdown_ref.py.

The tiny models and inputs are those of tests/separate_cases.py.  Both stages of a pair run at the input file's sample rate (a chain
refuses stages at different rates): ``sample_rate`` is the rate the plugins read and write at, the tiny nets do not care."""
import os
import random

import numpy as np
import pytest

from tests import separate_cases as SC
from tests.mixdown_ref import mixdown_ref
from tests.test_gpu_separate_rates import rewritten

pytestmark = pytest.mark.gpu

# (first family, the stem handed over, second family): each family once in either place
PAIRS = [("mdx", "Instrumental", "mdx"), ("mdxc", "s0", "vr"), ("demucs", "Vocals", "mdx"), ("vr", "Instrumental", "mdxc")]


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")


def plugin(family, tmp, sub, rate, **over):
    """A fresh plugin of the family's first golden case, writing into <tmp>/<sub>, at ``rate``."""
    tag, cls, common, arch, wav, _ = SC.cases(family, os.path.join(str(tmp), f"models_{family}"))[0]
    common = dict(common, output_dir=os.path.join(str(tmp), sub), sample_rate=rate, asx_profile_file=True, **over)
    return SC.plugin_class(cls)(common_config=common, arch_config=arch), wav


def golden_input(family, tmp):
    from audio_separator_amd import audio_io
    wav = SC.cases(family, os.path.join(str(tmp), f"models_{family}"))[0][4]
    return wav, audio_io.wav_info(wav)["samplerate"]


def stem_name_of(first, stem):
    """``stem`` may be a placeholder for "whatever the model calls its first stem" (the MDXC fixture's instrument names)."""
    if stem != "s0":
        return stem
    training = first.model_data.get("training", {})
    return training.get("target_instrument") or training["instruments"][0]


def blobs(out_dir, names):
    out = []
    for n in names:
        with open(os.path.join(out_dir, n), "rb") as f:
            out.append(f.read())
    return out


def literal(first, then, path, stem, custom=None):
    random.seed(4321)                                   # the Demucs shift offsets
    a = first.separate(path, custom)
    b = then.separate(os.path.join(first.output_dir, first.get_stem_output_path(stem, custom)), custom)
    return a + b


def chain_of(first, then, stem, **kw):
    from audio_separator_amd.workflow import ChainSeparator
    return ChainSeparator(first, then, stem, **kw)


def count_demix(plugin_instance):
    """how often the plugin closes its "demix" phase"""
    calls, real = [], plugin_instance._tick

    def tick(phase, t0):
        calls.append(phase)
        return real(phase, t0)
    plugin_instance._tick = tick
    return lambda: calls.count("demix")


def same_sources(a, b):
    for which in ("primary_source", "secondary_source"):
        x, y = getattr(a, which), getattr(b, which)
        assert (x is None) == (y is None), which
        if x is not None:
            assert np.array_equal(np.asarray(x), np.asarray(y)), which


def run_pair(tmp, f1, stem, f2, path, rate, over1=None, over2=None, **chain_kw):
    """The literal flow into <tmp>/lit and the chain into <tmp>/chain on fresh plugins; returns what both left."""
    over1, over2 = over1 or {}, over2 or dict(over1 or {})
    lit_first, _ = plugin(f1, tmp, "lit", rate, **over1)
    lit_then, _ = plugin(f2, tmp, "lit", rate, **over2)
    stem = stem_name_of(lit_first, stem)
    want = literal(lit_first, lit_then, path, stem)
    first, _ = plugin(f1, tmp, "chain", rate, **over1)
    then, _ = plugin(f2, tmp, "chain", rate, **over2)
    demixes = count_demix(first)
    chain = chain_of(first, then, stem.upper() if stem != "s0" else stem, **chain_kw)
    random.seed(4321)
    got = chain.separate(path)
    return {"want": want, "got": got, "chain": chain, "first": first, "then": then, "lit_first": lit_first, "lit_then": lit_then,
            "demixes": demixes(), "lit": os.path.join(str(tmp), "lit"), "out": os.path.join(str(tmp), "chain")}


def assert_device_and_equal(r, n_then_min=1):
    assert r["got"] == r["want"] and len(r["got"]) >= 1 + n_then_min
    assert r["chain"].last_path_taken == "device"
    assert blobs(r["out"], r["got"]) == blobs(r["lit"], r["want"])
    assert r["demixes"] == 1 and "demix" in r["first"].file_timings
    assert "read" not in r["then"].file_timings and "h2d_decode" not in r["then"].file_timings, r["then"].file_timings
    same_sources(r["first"], r["lit_first"])
    same_sources(r["then"], r["lit_then"])
    for key in ("audio_file_path", "input_bit_depth", "input_subtype", "_file_seconds", "_file_rate", "_file_frames", "wav_subtype",
                "input_audio_subtype"):                          # (the last two are VRSeparator's own)
        a, b = getattr(r["then"], key, None), getattr(r["lit_then"], key, None)
        assert (a.replace(r["out"], r["lit"]) if isinstance(a, str) and key == "audio_file_path" else a) == b, key


@pytest.mark.parametrize("f1,stem,f2", PAIRS)
def test_file_handoff_is_the_literal_flow(tmp_path, f1, stem, f2):
    path, rate = golden_input(f1, tmp_path)
    if "vr" in (f1, f2) and rate != 8000:
        # the VR fixture takes a device mix at its top band's rate, 8000 Hz: the same samples under that label
        path, rate = rewritten(SC.cases(f1, str(tmp_path / f"models_{f1}"))[0], tmp_path, 8000)[0], 8000
    r = run_pair(tmp_path, f1, stem, f2, path, rate)
    assert_device_and_equal(r)
    assert "read" in r["first"].file_timings                    # the input itself was read, once, by the first stage
    g = r["chain"].last_handoff_gain
    assert isinstance(g, float) and 0.0 < g <= 1.0


@pytest.mark.parametrize("subtype", ["PCM_16", "PCM_24"])
def test_flac_stems(tmp_path, subtype):
    """The default FLAC writer: a 16-bit stream, and the v << 8 24-bit stream of a 24-bit input; both read back as v / 2^15."""
    from audio_separator_amd import audio_io
    case = SC.cases("mdx", str(tmp_path / "models_mdx"))[0]
    path, _ = rewritten(case, tmp_path, 44100, subtype)
    r = run_pair(tmp_path, "mdx", "Instrumental", "mdxc", path, 44100, over1={"output_format": "FLAC"})
    assert_device_and_equal(r)
    assert all(n.endswith(".flac") for n in r["got"])
    info = audio_io.flac_stream(os.path.join(r["out"], r["got"][0]))
    assert info["bits_per_sample"] == (16 if subtype == "PCM_16" else 24)
    assert r["then"].input_bit_depth == info["bits_per_sample"]


@pytest.mark.parametrize("subtype", ["PCM_16", "PCM_24", "PCM_32", "FLOAT"])
def test_soundfile_wav_stems(tmp_path, subtype):
    """``use_soundfile``: the stem's file carries the input's own sample format, encoded on the device; the hand-off decodes those bytes."""
    from audio_separator_amd import audio_io
    case = SC.cases("mdx", str(tmp_path / "models_mdx"))[0]
    path, _ = rewritten(case, tmp_path, 44100, subtype)
    r = run_pair(tmp_path, "mdx", "Instrumental", "mdx", path, 44100, over1={"use_soundfile": True, "asx_output_encoder": "device"})
    assert_device_and_equal(r)
    assert r["first"].last_write_path == "wav_device_resident"
    for n in r["got"]:
        assert audio_io.wav_info(os.path.join(r["out"], n))["subtype"] == subtype, n


def test_input_at_another_rate(tmp_path):
    case = SC.cases("mdx", str(tmp_path / "models_mdx"))[0]
    path, _ = rewritten(case, tmp_path, 48000)
    r = run_pair(tmp_path, "mdx", "Instrumental", "mdx", path, 44100, over1={"asx_input_resample": "device"})
    assert_device_and_equal(r)
    assert "resample" in r["first"].file_timings and "resample" not in r["then"].file_timings


def test_flac_input(tmp_path):
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    wav, rate = golden_input("mdx", tmp_path)
    x, _ = audio_io.read_wav(wav)
    pcm = np.ascontiguousarray(np.rint(x.T * 32768.0).astype(np.int16))
    eng = A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))
    frames, sizes = eng.flac_encode(pcm, rate, 16)
    eng.close()
    path = str(tmp_path / "mdx_in.flac")
    audio_io.write_flac(path, frames, sizes, rate, 16, pcm.shape[0])
    r = run_pair(tmp_path, "mdx", "Instrumental", "mdx", path, rate)
    assert_device_and_equal(r)
    assert "flac_decode" in r["first"].file_timings


def test_fastpath_off_is_the_files_path_with_the_same_bytes(tmp_path, monkeypatch):
    path, rate = golden_input("mdx", tmp_path)
    dev = run_pair(tmp_path / "dev", "mdx", "Instrumental", "mdx", path, rate)
    assert dev["chain"].last_path_taken == "device"
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    off = run_pair(tmp_path / "off", "mdx", "Instrumental", "mdx", path, rate)
    assert off["chain"].last_path_taken == "files" and off["got"] == off["want"] == dev["got"]
    assert blobs(off["out"], off["got"]) == blobs(off["lit"], off["want"]) == blobs(dev["out"], dev["got"])


def test_float_handoff(tmp_path):
    """``then`` hears the normalised stem itself: the files of ``then.separate`` on a 32-bit float file of that stem.  With a FLOAT input
    the second stage's writer state is the same in both flows (the original input's = the float file's), so the bytes are.  The 16-bit
    hand-off gives other samples: the two modes are not one path."""
    from audio_separator_amd import audio_io
    case = SC.cases("mdx", str(tmp_path / "models_mdx"))[0]
    path, _ = rewritten(case, tmp_path, 44100, "FLOAT")
    # the flow through a float file: first.separate, the stem after the writer's normalise as FLOAT under the stem file's name
    lit_first, _ = plugin("mdx", tmp_path, "lit", 44100)
    lit_then, _ = plugin("mdx", tmp_path, "lit", 44100)
    a = lit_first.separate(path)
    stem_file = lit_first.get_stem_output_path("Instrumental", None)
    handed = np.array(lit_first.secondary_source, np.float32, copy=True)
    g = lit_first._normalize_factor(np.abs(handed).max())
    normalised = lit_first.engine.normalize(np.ascontiguousarray(handed), lit_first.normalization_threshold, lit_first.amplification_threshold)
    os.makedirs(tmp_path / "floatfile", exist_ok=True)
    audio_io.write_wav(str(tmp_path / "floatfile" / stem_file), normalised, 44100, "FLOAT")
    b = lit_then.separate(str(tmp_path / "floatfile" / stem_file))
    want = blobs(str(tmp_path / "lit"), b)

    first, _ = plugin("mdx", tmp_path, "chain", 44100)
    then, _ = plugin("mdx", tmp_path, "chain", 44100)
    chain = chain_of(first, then, "Instrumental", handoff="float")
    got = chain.separate(path)
    assert got == a + b and chain.last_path_taken == "device"
    assert g != 1.0 and chain.last_handoff_gain == g
    assert blobs(str(tmp_path / "chain"), got[len(a):]) == want
    assert "read" not in then.file_timings
    same_sources(then, lit_then)

    f_first, _ = plugin("mdx", tmp_path, "file", 44100)
    f_then, _ = plugin("mdx", tmp_path, "file", 44100)
    f_chain = chain_of(f_first, f_then, "Instrumental")
    f_got = f_chain.separate(path)
    assert f_got == got and f_chain.last_handoff_gain == g
    assert blobs(str(tmp_path / "file"), f_got[:len(a)]) == blobs(str(tmp_path / "chain"), got[:len(a)])       # the first stage's files agree
    assert blobs(str(tmp_path / "file"), f_got[len(a):]) != want                                               # the second stage's do not
    assert not np.array_equal(np.asarray(f_then.primary_source), np.asarray(then.primary_source))

    # the second stage's writer keeps the ORIGINAL input's format: a 16-bit input gives 16-bit second-stage stems
    p16, _ = golden_input("mdx", tmp_path)
    first16, _ = plugin("mdx", tmp_path, "f16", 44100)
    then16, _ = plugin("mdx", tmp_path, "f16", 44100)
    names = chain_of(first16, then16, "Instrumental", handoff="float").separate(p16)
    assert (then16.input_subtype, then16.input_bit_depth) == ("PCM_16", 16)
    assert all(audio_io.wav_info(os.path.join(str(tmp_path / "f16"), n))["subtype"] == "PCM_16" for n in names)


def test_separate_many_is_the_loop(tmp_path):
    """Three files of different lengths and one unreadable path: per file the bytes of ``ChainSeparator.separate``; the bad path fails alone."""
    from audio_separator_amd import audio_io
    wav, rate = golden_input("mdx", tmp_path)
    x, _ = audio_io.read_wav(wav)
    os.makedirs(tmp_path / "in", exist_ok=True)
    paths = []
    for i, n in enumerate((x.shape[1], 2011, 1024)):
        p = str(tmp_path / "in" / f"song{i}.wav")
        audio_io.write_wav(p, np.ascontiguousarray(x[:, :n].T), rate, "PCM_16")
        paths.append(p)
    paths.insert(2, str(tmp_path / "in" / "missing.wav"))
    mixdowns = {"Inst+Voc2": [("first", "Vocals", 1.0), ("then", "Vocals", 0.5)]}

    def stages(sub):
        first, _ = plugin("mdx", tmp_path, sub, rate)
        then, _ = plugin("mdx", tmp_path, sub, rate)
        return first, then, chain_of(first, then, "Instrumental", mixdowns=mixdowns)
    first, then, loop = stages("loop")
    want = []
    for p in paths:
        # between files the orchestrator resets the per-file state (MDXSeparator.separate honours sources that are already set)
        first.clear_file_specific_paths()
        then.clear_file_specific_paths()
        try:
            want.append(loop.separate(p))
        except Exception:
            want.append([])
    first_m, then_m, many = stages("many")
    got = many.separate_many(paths)
    assert got == want and got[2] == [] and all(len(g) == 5 for i, g in enumerate(got) if i != 2)
    assert sorted(many.batch_errors) == [2] and many.last_paths_taken == ["device", "device", "failed", "device"]
    for names in got:
        assert blobs(str(tmp_path / "many"), names) == blobs(str(tmp_path / "loop"), names)
    same_sources(first_m, first)
    same_sources(then_m, then)


def test_mixdown_is_the_writer_on_the_reference_sum(tmp_path):
    """"Instrumental + second-stage vocals" and a difference: each file is ``then``'s writer applied to mixdown_ref of the arrays the stages
    left in ``*_source``, the second stage's with w / g.  The handed stem peaks above ``normalization_threshold``: g != 1."""
    from audio_separator_amd.workflow import then_weight
    path, rate = golden_input("mdx", tmp_path)
    first, _ = plugin("mdx", tmp_path, "chain", rate)
    then, _ = plugin("mdx", tmp_path, "chain", rate)
    chain = chain_of(first, then, "Instrumental", mixdowns={"Mix": [("first", "Vocals", 1.0), ("then", "Instrumental", 0.8), ("then", "Vocals", -0.25)],
                                                            "Twice": [("first", "Instrumental", 2.0)]})
    got = chain.separate(path, {"twice": "two times"})
    assert chain.last_path_taken == "device"
    assert got[-2:] == ["mdx_in_(Mix)_net_small+net_small.wav", "two times.wav"] and len(got) == 6
    g = chain.last_handoff_gain
    assert g == first._normalize_factor(np.abs(first.secondary_source).max()) and g < 1.0
    n = first.primary_source.shape[0]
    want = {got[-2]: mixdown_ref([(first.primary_source, "rows", 1.0), (then.secondary_source, "rows", then_weight(0.8, g)),
                                  (then.primary_source, "rows", then_weight(-0.25, g))], n, "rows"),
            got[-1]: mixdown_ref([(first.secondary_source, "rows", 2.0)], n, "rows")}
    for name, ref in want.items():
        then.write_audio("expected.wav", ref)
        assert blobs(str(tmp_path / "chain"), [name]) == blobs(str(tmp_path / "chain"), ["expected.wav"]), name
