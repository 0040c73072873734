"""``common_config["asx_complement_rate"] = "input"``: with ``asx_output_rate="input"`` the complement stem's FILE -- the MDX secondary, the
residual row of a single-target MDXC / Roformer model -- is formed at the file's rate against the file's own decoded mix,

    c_f = fl( fl(s * mix_f) - fl(k * r) ),   r = the converted model stem, s = the mix normalise's factor, k = compensate | 1

so that the two written stems sum to s * the file (the null test), top band included.  What the plugin hands to ``write_audio`` and the
model stem's file stay as they are without the knob, bit for bit.

Inputs: the golden samples of tests/separate_cases.py under a 48 000 Hz (one: 96 000 Hz) header, as tests/test_gpu_separate_rates.py
``rewritten`` writes them, times ``gain``, plus 0.05 * sin at 0.47 of the file's rate (22.56 kHz at 48 kHz: above the converter's pass
band, so it reaches no stem at the model's rate) in both channels.

The null bound, 6 * 2^-24: the bound of tests/test_gpu_resample_complement.py minus the converter's term, which cancels because both files
carry the same r -- three float32 roundings are what is left of k * p + c - s * mix_f."""
import logging
import math
import os
import random

import numpy as np
import pytest

from tests import complement_ref as CR
from tests import resample_ref as RR
from tests import separate_cases as SC
from tests.test_gpu_separate_rates import separate_once

pytestmark = pytest.mark.gpu

THR, AMP = 0.9, 0.0                # normalization_threshold / amplification_threshold of tests/separate_cases.py common_config
TONE = 0.05
NULL_GAIN = 0.5                    # the null-test inputs: golden samples at half scale (mix peak about 0.5 + the tone)
ON = dict(asx_input_resample="device", asx_output_rate="input", asx_complement_rate="input")
OFF = dict(asx_input_resample="device", asx_output_rate="input")
CASES = ["mdx_plain", "mdxc_one", "rof"]


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


def case_by_tag(tag, tmp, **common_over):
    for family in ("mdx", "mdxc", "roformer"):
        for case in SC.cases(family, str(tmp)):
            if case[0] == tag:
                return (case[0], case[1], dict(case[2], **common_over), case[3], case[4], case[5])
    raise KeyError(tag)


def samples(case, rate, gain=1.0, burst=None):
    """float64 [2, F]: the golden samples repeated forwards and backwards (``rewritten``'s rule) times ``gain``, plus the tone; ``burst`` =
    (position as a fraction of the model-rate length, amplitude A): A * the sign pattern of the taps that the file -> model rate converter
    applies for one output sample, added to both channels over those taps' span.  That output then gains A * sum |taps| (2.5 A for 48 ->
    44.1 kHz) while no sample of the file moves by more than A: a mix whose peak at the model's rate lies well above its peak in the
    file (for the leg where the mix normalise engages and the stems must still stay below the writer's threshold)."""
    from audio_separator_amd import audio_io
    x, model_rate = audio_io.read_wav(case[4])
    reps = int(math.ceil(rate / model_rate))
    x = np.concatenate([x if r % 2 == 0 else x[:, ::-1] for r in range(reps)], axis=1).astype(np.float64) * gain
    F = x.shape[1]
    x += TONE * np.sin(2.0 * np.pi * 0.47 * np.arange(F))
    if burst is not None:
        L, M, half, _, h = RR.design(rate, model_rate)
        m0 = int(burst[0] * RR.plan_n_out(F, L, M))
        n = m0 * M - np.arange(F) * L                      # the tap input i meets at output m0: y[m0] = sum_i x[i] h[m0 M - i L]
        ok = np.abs(n) <= half
        x[:, ok] += burst[1] * np.sign(h[n[ok] + half])
    return x


def write_input(case, tmp, rate, subtype, gain=1.0, name=None, burst=None, tag=""):
    from audio_separator_amd import audio_io
    x = samples(case, rate, gain, burst)
    d = os.path.join(str(tmp), f"in_{rate}_{subtype}_{gain:g}{tag}")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, name or os.path.basename(case[4]))
    audio_io.write_wav(path, np.ascontiguousarray(x.T.astype(np.float32)), rate, subtype)
    return path, x.shape[1]


def mix_scale(eng, mix_f, rate, model_rate):
    """(s, the model-rate mix's peak): the factor the plugin's mix normalise applies, float32(0.9 / peak) as numpy forms it"""
    mix_m = eng.resample_rational(mix_f, rate, model_rate)
    peak = np.abs(mix_m).max()
    assert peak.dtype == np.float32
    return (np.float32(THR) / peak if peak > np.float32(THR) else np.float32(1.0)), float(peak)


def stem_scale(case):
    return case[2]["model_data"].get("compensate", 1.0) if case[1] == "MDXSeparator" else 1.0


def composed(eng, case, wav, calls):
    """(y, c, s): the converted model stem and the complement at the file's rate, from the public calls on what the plugin handed to
    write_audio (secondary = the complement first, then primary = the model stem) and the file as audio_io.read_wav decodes it; c with
    the MDXC per-stem normalise."""
    from audio_separator_amd import audio_io
    model_rate = case[2]["sample_rate"]
    mix_f, rate = audio_io.read_wav(wav)
    if mix_f.shape[0] == 1:
        mix_f = np.concatenate([mix_f, mix_f])
    s, _ = mix_scale(eng, mix_f, rate, model_rate)
    model_stem = calls[1][1]
    y, c = eng.resample_rational_complement(model_stem, model_rate, rate, mix_f.shape[1], mix_f, float(s), stem_scale(case), layout="rows")
    if case[1] == "MDXCSeparator":
        c = eng.normalize(c, THR, AMP)
    return y, c, s


def file_bytes(tmp, eng, stem, rate, writer):
    """The file ``writer`` makes of a planar stem [2, F]: "pcm16" / "pcm32" -- the pydub-less default writer on a 16-bit / 32-bit input;
    "float" -- ``use_soundfile`` on a FLOAT input (the device writer)."""
    from audio_separator_amd import audio_io
    path = str(tmp / "composed.wav")
    if writer == "float":
        body, peak = eng.pcm_encode(stem, "FLOAT", THR, AMP, layout="planar")
        audio_io.write_wav_body(path, body, rate, "FLOAT", stem.shape[1])
    else:
        pcm, peak = eng.pcm16(np.ascontiguousarray(stem.T), THR, AMP)
        audio_io.write_wav(path, pcm, rate, "PCM_16" if writer == "pcm16" else "PCM_32")
    assert peak >= 1e-6
    with open(path, "rb") as f:
        return f.read()


def check_composition(tmp, eng, case, wav, sub, writer, **over):
    """One run with the knob on against one with it off: names, every array handed to write_audio and the model stem's file are the
    same; the complement's file is the composition.  Returns (the knob-on run, the knob-off run)."""
    off = separate_once(case, wav, sub + "_off", **dict(OFF, **over))
    on = separate_once(case, wav, sub + "_on", **dict(ON, **over))
    names, calls, blobs, timings, _ = on
    assert names == off[0] and len(names) == len(calls) == 2
    assert "resample_out" in timings
    for (p, a), (p_off, b) in zip(calls, off[1]):
        assert p == p_off and a.shape == b.shape and np.array_equal(a, b)
    assert blobs[1] == off[2][1], "the model stem's file changed"
    assert blobs[0] != off[2][0], "the complement's file did not change"
    y, c, _ = composed(eng, case, wav, calls)
    from audio_separator_amd import audio_io
    rate = audio_io.wav_info(wav)["samplerate"]
    assert file_bytes(tmp, eng, c, rate, writer) == blobs[0], "complement"
    assert file_bytes(tmp, eng, y, rate, writer) == blobs[1], "model stem"
    return on, off


@pytest.mark.parametrize("tag,rate,subtype", [(t, 48000, st) for t in CASES for st in ("PCM_16", "FLOAT")] + [("mdx_plain", 96000, "PCM_16")])
def test_complement_file_is_the_composition_of_the_public_calls(tmp_path, monkeypatch, eng, tag, rate, subtype):
    case = case_by_tag(tag, tmp_path)
    wav, F = write_input(case, tmp_path, rate, subtype)
    on, _ = check_composition(tmp_path, eng, case, wav, "dflt", "pcm16" if subtype == "PCM_16" else "pcm32")
    # the host-array route (no device-resident decode, host stems) writes the same bytes
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    names_h, _, blobs_h, timings_h, _ = separate_once(case, wav, "hostpath", **ON)
    assert names_h == on[0] and blobs_h == on[2] and "h2d_decode" not in timings_h and "resample_out" in timings_h


def null_miss(case, out_sub, names, wav, s):
    """max |k * p + c - s * mix_f| over the two written FLOAT files, in float64; (miss, peak of p's file, peak of c's file)"""
    from audio_separator_amd import audio_io
    c, rate_c = audio_io.read_wav(os.path.join(case[2]["output_dir"], out_sub, names[0]))
    p, rate_p = audio_io.read_wav(os.path.join(case[2]["output_dir"], out_sub, names[1]))
    mix_f, rate = audio_io.read_wav(wav)
    assert rate_c == rate_p == rate and c.shape == p.shape == mix_f.shape
    k = float(np.float32(stem_scale(case)))
    total = k * p.astype(np.float64) + c.astype(np.float64)
    return float(np.abs(total - float(s) * mix_f.astype(np.float64)).max()), float(np.abs(p).max()), float(np.abs(c).max())


@pytest.mark.parametrize("tag", CASES)
def test_null_test_holds_at_the_files_rate(tmp_path, eng, tag):
    """use_soundfile on a FLOAT input: FLOAT stems through the device writer.  Preconditions (asserted; the input is scaled down until
    they hold): the mix normalise does not engage, and neither written stem reaches the writer's normalisation threshold."""
    from audio_separator_amd import audio_io
    case = case_by_tag(tag, tmp_path, use_soundfile=True, asx_output_encoder="device")
    gain = NULL_GAIN
    for _ in range(4):
        wav, F = write_input(case, tmp_path, 48000, "FLOAT", gain)
        mix_f, _ = audio_io.read_wav(wav)
        s, mix_peak = mix_scale(eng, mix_f, 48000, case[2]["sample_rate"])
        names, calls, blobs, _, _ = separate_once(case, wav, f"null_{gain:g}", **ON)
        y, c, _ = composed(eng, case, wav, calls)
        peaks = float(np.abs(y).max()), float(np.abs(c).max())
        print(f"{tag}: gain {gain:g}: model-rate mix peak {mix_peak:.4f}, stems at the file's rate peak {peaks[0]:.4f} / {peaks[1]:.4f}")
        if mix_peak <= THR and max(peaks) < THR:
            break
        gain *= 0.5
    assert s == 1.0 and mix_peak <= THR and max(peaks) < THR, (gain, mix_peak, peaks)
    assert len(names) == 2 and all(audio_io.wav_info(os.path.join(case[2]["output_dir"], f"null_{gain:g}", n))["subtype"] == "FLOAT" for n in names)
    miss, p_peak, c_peak = null_miss(case, f"null_{gain:g}", names, wav, s)
    print(f"{tag}: null test with the knob on: max |k p + c - mix_f| = {miss:.3e} (bound {CR.ROUNDING_BOUND:.3e})")
    assert p_peak < THR and c_peak < THR
    assert miss <= CR.ROUNDING_BOUND, miss
    # the files are the composition here as well (the device FLOAT writer)
    assert file_bytes(tmp_path, eng, c, 48000, "float") == blobs[0] and file_bytes(tmp_path, eng, y, 48000, "float") == blobs[1]
    # ... and without the knob the same sum misses by the band above the converter's pass band: the test can see the difference
    names_off, _, _, _, _ = separate_once(case, wav, "null_off", **OFF)
    miss_off, _, _ = null_miss(case, "null_off", names_off, wav, s)
    print(f"{tag}: null test with the knob off: {miss_off:.3e}")
    assert miss_off > 0.02, miss_off


def test_null_test_against_the_scaled_file_when_the_mix_normalise_engages(tmp_path, eng):
    """A mix whose peak lies above 0.9: the null holds against s * mix_f, s = float32(0.9 / peak) as numpy forms it.  The written stems must
    still stay below the writer's threshold, and the complement is about s * mix_f where the model's stem is small: so the input is quiet
    material (the golden samples at 0.1) whose model-rate peak comes from ``samples``' sign pattern -- 0.37 * 2.55 = 0.94 plus the
    material, against 0.37 + 0.1 + 0.05 in the file.  A few amplitudes are tried until both preconditions hold; they are asserted."""
    from audio_separator_amd import audio_io
    case = case_by_tag("mdx_plain", tmp_path, use_soundfile=True, asx_output_encoder="device")
    found = None
    for i, burst in enumerate([(0.5, 0.37), (0.5, 0.4), (0.3, 0.37), (0.5, 0.45), (0.7, 0.4)]):
        wav, F = write_input(case, tmp_path, 48000, "FLOAT", 0.1, burst=burst, tag=f"_b{i}")
        mix_f, _ = audio_io.read_wav(wav)
        s, mix_peak = mix_scale(eng, mix_f, 48000, case[2]["sample_rate"])
        names, calls, blobs, _, _ = separate_once(case, wav, f"burst{i}", **ON)
        y, c, _ = composed(eng, case, wav, calls)
        peaks = float(np.abs(y).max()), float(np.abs(c).max())
        print(f"burst {burst}: model-rate mix peak {mix_peak:.4f}, s {float(s):.6f}, stems at the file's rate peak {peaks[0]:.4f} / {peaks[1]:.4f}")
        if mix_peak > THR and max(peaks) < THR:
            found = (i, wav, names, s)
            break
    assert found is not None, "no input with a mix peak above 0.9 and both stems below it"
    i, wav, names, s = found
    assert s < 1.0 and s == np.float32(THR) / np.float32(mix_peak)
    miss, p_peak, c_peak = null_miss(case, f"burst{i}", names, wav, s)
    print(f"null test against s * mix_f: {miss:.3e} (bound {CR.ROUNDING_BOUND:.3e})")
    assert p_peak < THR and c_peak < THR and miss <= CR.ROUNDING_BOUND, (miss, p_peak, c_peak)


@pytest.mark.parametrize("tag", CASES)
def test_flac_input_gives_the_bytes_of_the_wav_input(tmp_path, eng, tag):
    from audio_separator_amd import audio_io
    case = case_by_tag(tag, tmp_path)
    wav, F = write_input(case, tmp_path, 48000, "PCM_16")
    with open(wav, "rb") as f:
        info = audio_io.wav_info(wav)
        f.seek(info["data_offset"])
        pcm = np.frombuffer(f.read(F * 4), "<i2").reshape(F, 2)
    frames, sizes = eng.flac_encode(pcm, 48000, 16)
    d = tmp_path / "flac_in"
    d.mkdir()
    flac = str(d / (os.path.splitext(os.path.basename(wav))[0] + ".flac"))
    audio_io.write_flac(flac, frames, sizes, 48000, 16, F, None, block_size=eng.FLAC_BLOCK_SIZE)
    names_w, _, blobs_w, _, _ = separate_once(case, wav, "from_wav", **ON)
    names_f, _, blobs_f, timings_f, _ = separate_once(case, flac, "from_flac", **ON)
    assert "flac_decode" in timings_f and names_f == names_w and blobs_f == blobs_w


@pytest.mark.parametrize("tag", CASES)
def test_separate_many_writes_what_separate_writes_and_releases_the_mixes(tmp_path, tag):
    case = case_by_tag(tag, tmp_path)
    _, cls, common, arch, _, _ = case
    rates = (common["sample_rate"], 48000, 96000)
    files = [write_input(case, tmp_path, rate, "PCM_16", name=f"song{rate}.wav")[0] for rate in rates]

    def run(out_sub, many, **over):
        out_dir = os.path.join(common["output_dir"], out_sub)
        inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, **over), arch_config=arch)
        random.seed(4321)
        if many:
            results = inst.separate_many(files)
            assert inst.batch_errors == {}, inst.batch_errors
            assert inst._file_mix is None and inst._complement is None        # the kept mixes are gone with the last file's write
        else:
            results = []
            for f in files:
                results.append(inst.separate(f, None))
                assert inst._file_mix is None and inst._complement is None
                inst.clear_file_specific_paths()
        blobs = []
        for names in results:
            assert len(names) == 2
            for n in names:
                with open(os.path.join(out_dir, n), "rb") as f:
                    blobs.append((n, f.read()))
        inst.clear_gpu_cache()
        return blobs

    one, many, off = run("one", False, **ON), run("many", True, **ON), run("off", False, **OFF)
    assert [n for n, _ in one] == [n for n, _ in many] == [n for n, _ in off] and len({n for n, _ in one}) == len(one)
    for (n, a), (_, b) in zip(one, many):
        assert a == b, n
    # the file at the model's rate is written as without the knob; of the others the complement (first of each pair) differs
    assert [a == b for (_, a), (_, b) in zip(one, off)] == [True, True, False, True, False, True]


def test_single_stem_naming_the_model_stem_keeps_nothing(tmp_path):
    for tag, stem in (("mdx_plain", "Vocals"), ("mdxc_one", "Vocals")):
        case = case_by_tag(tag, tmp_path, output_single_stem=stem)
        wav, _ = write_input(case, tmp_path, 48000, "PCM_16")
        _, cls, common, arch, _, _ = case
        inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=os.path.join(common["output_dir"], "single_on"), **ON), arch_config=arch)
        kept = []
        real = inst.write_audio
        inst.write_audio = lambda path, source: (kept.append(inst._file_mix), real(path, source))[1]
        names = inst.separate(wav, None)
        assert len(names) == 1 and kept == [None] and inst._file_mix is None and inst._complement is None
        with open(os.path.join(common["output_dir"], "single_on", names[0]), "rb") as f:
            blob = f.read()
        inst.clear_gpu_cache()
        names_off, _, blobs_off, _, _ = separate_once(case, wav, "single_off", **OFF)
        assert names_off == names and blobs_off == [blob]


def test_single_stem_naming_the_complement_writes_the_same_complement(tmp_path):
    """only the complement is wanted: the launch stores no converted model stem, and the file is the one of the two-stem run"""
    both = case_by_tag("mdx_plain", tmp_path)
    wav, _ = write_input(both, tmp_path, 48000, "PCM_16")
    names, _, blobs, _, _ = separate_once(both, wav, "both", **ON)
    single = case_by_tag("mdx_plain", tmp_path, output_single_stem="Instrumental")
    names_s, _, blobs_s, _, _ = separate_once(single, wav, "single", **ON)
    assert names_s == names[:1] and blobs_s == blobs[:1]


def test_a_model_without_a_complement_writes_todays_bytes_and_says_so_once(tmp_path, caplog):
    case = case_by_tag("mdxc_two", tmp_path)
    wav, _ = write_input(case, tmp_path, 48000, "PCM_16")
    _, cls, common, arch, _, _ = case
    out_dir = os.path.join(common["output_dir"], "two_on")
    logger = logging.getLogger("asx_complement_rate_test")
    inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, logger=logger, **ON), arch_config=arch)
    with caplog.at_level(logging.INFO, logger="asx_complement_rate_test"):
        first = inst.separate(wav, None)
        inst.clear_file_specific_paths()
        second = inst.separate(wav, None)
    notes = [r for r in caplog.records if "asx_complement_rate='input' does nothing" in r.getMessage()]
    assert len(notes) == 1 and first == second and inst._file_mix is None
    blobs = []
    for n in first:
        with open(os.path.join(out_dir, n), "rb") as f:
            blobs.append(f.read())
    inst.clear_gpu_cache()
    names_off, _, blobs_off, _, _ = separate_once(case, wav, "two_off", **OFF)
    assert names_off == first and blobs_off == blobs


@pytest.mark.parametrize("tag", ["mdx_plain", "mdxc_one"])
def test_a_file_at_the_models_rate_writes_todays_bytes(tmp_path, tag):
    case = case_by_tag(tag, tmp_path)
    names, _, blobs, _, _ = separate_once(case, case[4], "plain")
    names_on, _, blobs_on, timings, _ = separate_once(case, case[4], "knob", **ON)
    assert names_on == names and blobs_on == blobs and "resample_out" not in timings


def test_pitch_shift_keeps_the_algebra(tmp_path, eng):
    """the residual with pitch_shift is taken against the original mix: the same composition"""
    tag, cls, common, arch, wav0, custom = case_by_tag("mdxc_one", tmp_path)
    case = (tag, cls, common, dict(arch, pitch_shift=2), wav0, custom)
    wav, _ = write_input(case, tmp_path, 48000, "PCM_16")
    check_composition(tmp_path, eng, case, wav, "pitch", "pcm16")


def host_loader(eng):
    """A stand-in for librosa.load behind audio_io.load (librosa is optional, and this project's own host loader refuses another rate and
    FLAC): the file at its own rate -- RIFF/WAVE through read_wav, FLAC through Engine.flac_decode -- or converted to ``sr`` with
    Engine.resample_rational, so that the host decoder gives the model-rate mix of the device route and the files can be compared."""
    from audio_separator_amd import audio_io

    def load(path, sr=44100, mono=False, res_type=None):
        if audio_io.is_flac(path):
            info = audio_io.flac_stream(path)
            with open(path, "rb") as f:
                x, file_sr = eng.flac_decode(f.read()[info["audio_offset"]:], info), info["samplerate"]
        else:
            x, file_sr = audio_io.read_wav(path)
        if sr is not None and sr != file_sr:
            x, file_sr = eng.resample_rational(x, file_sr, sr), sr
        return (x[0] if x.shape[0] == 1 else x), file_sr
    return load


@pytest.mark.parametrize("leg", ["wav_host_decoder", "flac_without_the_device_file_path"])
@pytest.mark.parametrize("tag", ["mdx_plain", "mdxc_one"])
def test_a_file_the_host_decoder_converts_gets_the_same_complement(tmp_path, monkeypatch, eng, tag, leg):
    """The knob does not depend on who converts the input: with asx_input_resample="host" (the default), and for a FLAC file under
    ASX_FILE_FASTPATH=0, prepare_mix decodes the file once more at its own rate and keeps it.  With a host decoder that converts like
    the device does, the files are those of the device route."""
    from audio_separator_amd import audio_io
    case = case_by_tag(tag, tmp_path)
    wav, F = write_input(case, tmp_path, 48000, "PCM_16")
    names_dev, _, blobs_dev, _, _ = separate_once(case, wav, "dev", **ON)
    names_off, _, blobs_off, _, _ = separate_once(case, wav, "dev_off", **OFF)
    assert blobs_dev[0] != blobs_off[0] and blobs_dev[1] == blobs_off[1]
    monkeypatch.setattr(audio_io, "load", host_loader(eng))
    if leg == "wav_host_decoder":
        path, over = wav, dict(ON, asx_input_resample="host")
    else:
        with open(wav, "rb") as f:
            f.seek(audio_io.wav_info(wav)["data_offset"])
            pcm = np.frombuffer(f.read(F * 4), "<i2").reshape(F, 2)
        frames, sizes = eng.flac_encode(pcm, 48000, 16)
        d = tmp_path / "flac_in"
        d.mkdir()
        path = str(d / (os.path.splitext(os.path.basename(wav))[0] + ".flac"))
        audio_io.write_flac(path, frames, sizes, 48000, 16, F, None, block_size=eng.FLAC_BLOCK_SIZE)
        monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
        over = ON
    names, _, blobs, timings, _ = separate_once(case, path, "host_decoded", **over)
    assert "h2d_decode" not in timings and "flac_decode" not in timings and "resample_out" in timings
    assert names == names_dev and blobs == blobs_dev


@pytest.mark.parametrize("tag", ["mdx_plain", "mdxc_one"])
def test_separate_many_without_the_device_file_path(tmp_path, monkeypatch, tag):
    """ASX_FILE_FASTPATH=0: host-decoded mixes and host arrays kept per file (MDX still pools on the device and reads s there): the bytes
    of the loop of ``separate`` on the same route, which are those of the device route"""
    case = case_by_tag(tag, tmp_path)
    _, cls, common, arch, _, _ = case
    files = [write_input(case, tmp_path, rate, "PCM_16", name=f"song{rate}.wav")[0] for rate in (common["sample_rate"], 48000, 96000)]

    def run(out_sub, many):
        out_dir = os.path.join(common["output_dir"], out_sub)
        inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, **ON), arch_config=arch)
        if many:
            results = inst.separate_many(files)
            assert inst.batch_errors == {}, inst.batch_errors
        else:
            results = []
            for f in files:
                results.append(inst.separate(f, None))
                inst.clear_file_specific_paths()
        assert inst._file_mix is None and inst._complement is None
        blobs = []
        for names in results:
            assert len(names) == 2
            for n in names:
                with open(os.path.join(out_dir, n), "rb") as f:
                    blobs.append(f.read())
        inst.clear_gpu_cache()
        return blobs
    device_route = run("fast_one", False)
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    one, many = run("host_one", False), run("host_many", True)
    assert one == many and one == device_route


def test_stems_dev_keeps_nothing(tmp_path):
    """stems_dev / stems_dev_many write nothing: no file-rate mix is kept"""
    for tag in ("mdx_plain", "mdxc_one"):
        case = case_by_tag(tag, tmp_path)
        _, cls, common, arch, _, _ = case
        wav, _ = write_input(case, tmp_path, 48000, "PCM_16")
        inst = SC.plugin_class(cls)(common_config=dict(common, **ON), arch_config=arch)
        kept = []
        real = inst._device_mix
        inst._device_mix = lambda *a, **k: (lambda m: (kept.append(inst._file_mix), m)[1])(real(*a, **k))
        stems = inst.stems_dev(wav)
        assert stems and inst._file_mix is None
        many, states = inst.stems_dev_many([wav, wav])
        assert all(isinstance(s, list) for s in many) and all(st["_file_mix"] is None for st in states)
        assert kept and all(k is None for k in kept) and inst._file_mix is None
        inst.clear_gpu_cache()
