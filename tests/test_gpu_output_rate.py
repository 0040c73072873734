"""``common_config["asx_output_rate"] = "input"``: stems written at the input file's own sample rate with exactly its frame count, for
MDXSeparator, MDXCSeparator (TFC-TDF and Roformer) and DemucsSeparator -- ``separate`` and ``separate_many``, WAV and FLAC, the pydub-less
default writer and ``use_soundfile``, the device-resident route and the host-array route.  With the knob absent, or "model", or a file
already at the model's rate, the bytes are the ones written without it.

The inputs are the golden inputs of tests/separate_cases.py rewritten at 48 000 Hz (one at 96 000 Hz) by the helper of
tests/test_gpu_separate_rates.py, entering with ``asx_input_resample="device"``."""
import os
import random

import numpy as np
import pytest

from tests import resample_ref as RR
from tests import separate_cases as SC
from tests.test_gpu_separate_rates import FAMILIES, case_of, rewritten, separate_once

pytestmark = pytest.mark.gpu


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


def out_path(case, sub, name):
    return os.path.join(case[2]["output_dir"], sub, name)


@pytest.mark.parametrize("family", FAMILIES)
def test_knob_absent_or_model_writes_todays_bytes(tmp_path, family):
    case = case_of(family, tmp_path)
    wav, _ = rewritten(case, tmp_path, 48000)
    names, calls, blobs, timings, _ = separate_once(case, wav, "absent", asx_input_resample="device")
    names_m, calls_m, blobs_m, timings_m, _ = separate_once(case, wav, "model", asx_input_resample="device", asx_output_rate="model")
    assert names_m == names and blobs_m == blobs
    assert "resample_out" not in timings and "resample_out" not in timings_m


@pytest.mark.parametrize("family", FAMILIES)
def test_a_file_at_the_models_rate_is_written_as_before(tmp_path, family):
    case = case_of(family, tmp_path)
    names, _, blobs, _, _ = separate_once(case, case[4], "off")
    names_i, _, blobs_i, timings_i, _ = separate_once(case, case[4], "on", asx_output_rate="input")
    assert names_i == names and blobs_i == blobs
    assert "resample_out" not in timings_i


@pytest.mark.parametrize("family,rate", [(f, 48000) for f in FAMILIES] + [("mdx", 96000)])
def test_input_rate_wav(tmp_path, monkeypatch, eng, family, rate):
    from audio_separator_amd import audio_io
    case = case_of(family, tmp_path)
    common = case[2]
    model_rate = common["sample_rate"]
    wav, F = rewritten(case, tmp_path, rate)
    n_model = -(-F * model_rate // rate)

    names_off, calls_off, _, _, _ = separate_once(case, wav, "off", asx_input_resample="device")
    names, calls, blobs, timings, _ = separate_once(case, wav, "on", asx_input_resample="device", asx_output_rate="input")
    assert names == names_off and len(calls) == len(names) > 0
    assert "resample_out" in timings and "resample" in timings, timings
    # what the plugin hands to write_audio stays at the model's rate, bit for bit
    for (p, a), (p_off, b) in zip(calls, calls_off):
        assert p == p_off and a.shape == b.shape == (n_model, 2) and np.array_equal(a, b)
    for n, (_, arr), blob in zip(names, calls, blobs):
        info = audio_io.wav_info(out_path(case, "on", n))
        assert (info["samplerate"], info["frames"], info["subtype"]) == (rate, F, "PCM_16"), n
        # the file is the composition of the public calls on that array
        n_out = RR.output_frames(arr.shape[0], F, rate, model_rate)
        assert n_out == F
        y = eng.resample_rational_stem(arr, model_rate, rate, n_out, layout="rows")
        pcm, peak = eng.pcm16(np.ascontiguousarray(y.T), common["normalization_threshold"], common["amplification_threshold"])
        assert peak >= 1e-6
        composed = str(tmp_path / "composed.wav")
        audio_io.write_wav(composed, pcm, rate, "PCM_16")
        with open(composed, "rb") as f:
            assert f.read() == blob, n

    # the host-array route (no device-resident decode, host stems) writes the same bytes
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    names_h, calls_h, blobs_h, timings_h, _ = separate_once(case, wav, "hostpath", asx_input_resample="device", asx_output_rate="input")
    assert names_h == names and blobs_h == blobs and "resample_out" in timings_h and "h2d_decode" not in timings_h


@pytest.mark.parametrize("family", FAMILIES)
def test_input_rate_flac(tmp_path, eng, family):
    from audio_separator_amd import audio_io
    case = case_of(family, tmp_path)
    wav, F = rewritten(case, tmp_path, 48000)
    names_w, _, _, _, _ = separate_once(case, wav, "wav", asx_input_resample="device", asx_output_rate="input")
    names_f, _, blobs_f, _, _ = separate_once(case, wav, "flac", asx_input_resample="device", asx_output_rate="input", output_format="FLAC")
    assert [os.path.splitext(n)[0] for n in names_f] == [os.path.splitext(n)[0] for n in names_w] and names_f
    for nw, nf, data in zip(names_w, names_f, blobs_f):
        path = out_path(case, "flac", nf)
        assert audio_io.is_flac(path)
        info = audio_io.flac_stream(path)
        assert (info["samplerate"], info["total_samples"], info["channels"], info["bits_per_sample"]) == (48000, F, 2, 16), nf
        mix = eng.flac_decode(data[info["audio_offset"]:], info)
        samples, rate = audio_io.read_wav(out_path(case, "wav", nw))
        assert rate == 48000 and mix.shape == samples.shape == (2, F)
        assert np.array_equal(mix, samples), nf


@pytest.mark.parametrize("family", ["mdx", "demucs"])
def test_use_soundfile_keeps_the_subtype_at_the_input_rate(tmp_path, family):
    from audio_separator_amd import audio_io
    case = case_of(family, tmp_path)
    wav, F = rewritten(case, tmp_path, 48000, "PCM_24")
    names, _, _, timings, state = separate_once(case, wav, "sf", asx_input_resample="device", asx_output_rate="input", use_soundfile=True)
    assert names and state[:2] == ("PCM_24", 24) and "resample_out" in timings
    for n in names:
        info = audio_io.wav_info(out_path(case, "sf", n))
        assert (info["samplerate"], info["frames"], info["subtype"]) == (48000, F, "PCM_24"), n


def test_mdx_invert_using_spec_secondary_follows_the_length_rule(tmp_path):
    from audio_separator_amd import audio_io
    case = case_of("mdx", tmp_path)
    wav, F = rewritten(case, tmp_path, 48000)
    names, calls, _, _, _ = separate_once(case, wav, "inv", asx_input_resample="device", asx_output_rate="input", invert_using_spec=True)
    n_model = -(-F * 147 // 160)
    lengths = sorted(arr.shape[0] for _, arr in calls)
    assert lengths == [1024 * (n_model // 1024), n_model] and lengths[0] < lengths[1]
    for n, (_, arr) in zip(names, calls):
        want = RR.output_frames(arr.shape[0], F, 48000, 44100)
        assert want == (F if arr.shape[0] == n_model else -(-arr.shape[0] * 160 // 147)) and want <= F
        info = audio_io.wav_info(out_path(case, "inv", n))
        assert (info["samplerate"], info["frames"]) == (48000, want), n


@pytest.mark.parametrize("family", FAMILIES)
def test_separate_many_writes_what_separate_writes(tmp_path, family):
    """[48 kHz, the model's rate, 96 kHz] in one pooled call: per file the bytes of ``separate`` (the Demucs shift offsets are drawn in
    file order, so both runs start from one seed)."""
    from audio_separator_amd import audio_io
    case = case_of(family, tmp_path)
    tag, cls, common, arch, _, _ = case
    rates = (48000, common["sample_rate"], 96000)
    files = [rewritten(case, tmp_path, rate, name=f"song{rate}.wav") for rate in rates]

    def run(out_sub, many):
        out_dir = os.path.join(common["output_dir"], out_sub)
        inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, asx_input_resample="device", asx_output_rate="input"),
                                    arch_config=arch)
        random.seed(4321)
        if many:
            results = inst.separate_many([f for f, _ in files])
            assert inst.batch_errors == {}, inst.batch_errors
        else:
            results = []
            for f, _ in files:
                results.append(inst.separate(f, None))
                inst.clear_file_specific_paths()
        blobs = []
        for names, (_, frames), rate in zip(results, files, rates):
            assert names
            for n in names:
                info = audio_io.wav_info(os.path.join(out_dir, n))
                assert (info["samplerate"], info["frames"]) == (rate, frames), n
                with open(os.path.join(out_dir, n), "rb") as f:
                    blobs.append((n, f.read()))
        inst.clear_gpu_cache()
        return blobs

    one, many = run("one", False), run("many", True)
    assert [n for n, _ in one] == [n for n, _ in many] and len({n for n, _ in one}) == len(one)
    for (n, a), (_, b) in zip(one, many):
        assert a == b, n


def test_refusals(tmp_path):
    from audio_separator_amd.ensemble import EnsembleSeparator
    mdx, mdxc, vr = case_of("mdx", tmp_path), case_of("mdxc", tmp_path), case_of("vr", tmp_path)

    def member(case, **over):
        tag, cls, common, arch, _, _ = case
        return SC.plugin_class(cls)(common_config=dict(common, **over), arch_config=arch)
    with pytest.raises(ValueError, match="asx_output_rate must be one of"):
        member(mdx, asx_output_rate="gpu")
    with pytest.raises(ValueError, match="asx_output_rate='input' is not supported by VRSeparator"):
        member(vr, asx_output_rate="input")
    member(vr, asx_output_rate="model")
    with pytest.raises(ValueError, match="asx_output_rate='input' is not supported in an ensemble"):
        EnsembleSeparator([member(mdx), member(mdxc, asx_output_rate="input")])
    EnsembleSeparator([member(mdx), member(mdxc, asx_output_rate="model")])
