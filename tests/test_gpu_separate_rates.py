"""Input files at another sample rate than the model's, with ``common_config["asx_input_resample"] = "device"``: the RIFF/WAVE file is
decoded at its own frame count and brought to the model's rate by asx_resample_rational_dev, for MDXSeparator, MDXCSeparator (TFC-TDF
and Roformer) and DemucsSeparator -- ``separate``, ``separate_many`` and the ensemble.  Without the knob such a file behaves as before.

The inputs are the golden inputs of tests/separate_cases.py rewritten at 48 000 Hz (and 96 000 Hz) with audio_io.write_wav: the same
samples, repeated forwards and backwards until the converted file is at least as long as the golden one (the Roformer case refuses a
mix shorter than a chunk)."""
import math
import os
import random

import numpy as np
import pytest

from tests import separate_cases as SC

pytestmark = pytest.mark.gpu

FAMILIES = ["mdx", "mdxc", "roformer", "demucs"]


def case_of(family, tmp):
    return SC.cases(family, str(tmp))[0]


def rewritten(case, tmp, rate, subtype="PCM_16", channels=2, name=None):
    """The case's golden input as a file at ``rate`` Hz, under the golden file's base name unless ``name`` is given; returns
    (path, frames)."""
    from audio_separator_amd import audio_io
    x, model_rate = audio_io.read_wav(case[4])
    reps = int(math.ceil(rate / model_rate))
    x = np.concatenate([x if r % 2 == 0 else x[:, ::-1] for r in range(reps)], axis=1)[:channels]
    d = os.path.join(str(tmp), f"in_{rate}_{subtype}_{channels}")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, name or os.path.basename(case[4]))
    audio_io.write_wav(path, np.ascontiguousarray(x.T), rate, subtype)
    return path, x.shape[1]


def separate_once(case, wav, out_sub, **common_over):
    """One fresh plugin, one ``separate``: (names, [(name, array handed to write_audio)], file bytes, file_timings,
    (input_subtype, input_bit_depth, _file_seconds) as the file left them)."""
    tag, cls, common, arch, _, _ = case
    common = dict(common, asx_profile_file=True, output_dir=os.path.join(common["output_dir"], out_sub), **common_over)
    inst = SC.plugin_class(cls)(common_config=common, arch_config=arch)
    calls = []
    real_write = inst.write_audio

    def write_audio(stem_path, stem_source):
        calls.append((stem_path, np.array(stem_source, copy=True)))
        real_write(stem_path, stem_source)
    inst.write_audio = write_audio
    random.seed(4321)                                   # the Demucs shift offsets
    names = inst.separate(wav, None)
    timings = dict(inst.file_timings)
    state = (inst.input_subtype, inst.input_bit_depth, inst._file_seconds)
    blobs = []
    for n in names:
        with open(os.path.join(common["output_dir"], n), "rb") as f:
            blobs.append(f.read())
    inst.clear_gpu_cache()
    inst.clear_file_specific_paths()
    return names, calls, blobs, timings, state


@pytest.mark.parametrize("family", FAMILIES)
def test_without_the_knob_the_file_behaves_as_before(tmp_path, monkeypatch, family):
    from audio_separator_amd import audio_io
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    case = case_of(family, tmp_path)
    wav, _ = rewritten(case, tmp_path, 48000)
    if audio_io._optional("librosa") is None:
        for over in ({}, {"asx_input_resample": "host"}):
            with pytest.raises(audio_io.AudioIOError, match="48000 Hz"):
                separate_once(case, wav, "host", **over)
    else:
        _, _, _, timings, _ = separate_once(case, wav, "host")
        assert "resample" not in timings
    with pytest.raises(ValueError, match="asx_input_resample"):
        separate_once(case, wav, "bad", asx_input_resample="gpu")


@pytest.mark.parametrize("subtype,channels", [("PCM_16", 2), ("FLOAT", 1)])
@pytest.mark.parametrize("family", FAMILIES)
def test_device_resample_file_path(tmp_path, monkeypatch, family, subtype, channels):
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    case = case_of(family, tmp_path)
    model_rate = case[2]["sample_rate"]
    wav, frames = rewritten(case, tmp_path, 48000, subtype, channels)
    g = math.gcd(48000, model_rate)
    n_out = -(-frames * (model_rate // g) // (48000 // g))

    usual, _, _, _, _ = separate_once(case, case[4], "usual")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    names, calls, blobs, timings, state = separate_once(case, wav, "dev", asx_input_resample="device")
    assert names == usual and len(calls) == len(names)
    assert "h2d_decode" in timings and "resample" in timings, timings
    assert all(arr.shape == (n_out, 2) for _, arr in calls)
    assert state == (subtype, 16 if subtype == "PCM_16" else 32, frames / 48000.0)
    for n in names:
        info = audio_io.wav_info(os.path.join(case[2]["output_dir"], "dev", n))
        assert info["samplerate"] == model_rate and info["frames"] == n_out

    # the host path (no device-resident decode) converts with the same kernel: equal arrays, equal files
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    names_h, calls_h, blobs_h, timings_h, state_h = separate_once(case, wav, "hostpath", asx_input_resample="device")
    assert "h2d_decode" not in timings_h and "resample" in timings_h, timings_h
    assert names_h == names and state_h[:2] == state[:2]
    for (_, a), (_, b) in zip(calls, calls_h):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert blobs_h == blobs
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")

    # accuracy: the plugin on the array Engine.resample_rational prepares from the decoded file (handed over as a float32 file at the model's rate)
    x, rate = audio_io.read_wav(wav)
    eng = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    y = eng.resample_rational(x, rate, model_rate)
    eng.close()
    assert y.shape == (channels, n_out)
    prepared = os.path.join(str(tmp_path), "prepared", os.path.basename(wav))
    os.makedirs(os.path.dirname(prepared), exist_ok=True)
    audio_io.write_wav(prepared, np.ascontiguousarray(y.T), model_rate, "FLOAT")
    names_p, calls_p, _, timings_p, _ = separate_once(case, prepared, "prepared")
    assert names_p == names and "resample" not in timings_p
    for (p, a), (_, b) in zip(calls, calls_p):
        err = SC.rel_rms(a, b)
        print(f"{family} {subtype} x{channels} {p}: rel rms vs the prepared array {err:.3e}")
        assert err < SC.TOL_STEM, (p, err)


def test_environment_overrides_the_configuration(tmp_path, monkeypatch):
    case = case_of("mdx", tmp_path)
    wav, _ = rewritten(case, tmp_path, 48000)
    monkeypatch.setenv("ASX_INPUT_RESAMPLE", "device")
    _, _, blobs_env, timings, _ = separate_once(case, wav, "env", asx_input_resample="host")
    assert "resample" in timings
    monkeypatch.delenv("ASX_INPUT_RESAMPLE")
    _, _, blobs_cfg, _, _ = separate_once(case, wav, "cfg", asx_input_resample="device")
    assert blobs_env == blobs_cfg


def test_a_pair_the_converter_refuses_and_a_silent_file(tmp_path, monkeypatch):
    from audio_separator_amd import audio_io
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    case = case_of("mdx", tmp_path)
    odd, _ = rewritten(case, tmp_path, 44056)
    if audio_io._optional("librosa") is None:
        with pytest.raises(audio_io.AudioIOError, match="44056 Hz"):           # as without the knob
            separate_once(case, odd, "odd", asx_input_resample="device")
    silent = str(tmp_path / "silent48.wav")
    audio_io.write_wav(silent, np.zeros((4000, 2), np.int16), 48000, "PCM_16")
    for fast in ("1", "0"):
        monkeypatch.setenv("ASX_FILE_FASTPATH", fast)
        with pytest.raises(ValueError, match="empty or not valid"):
            separate_once(case, silent, "silent", asx_input_resample="device")


@pytest.mark.parametrize("family", FAMILIES)
def test_separate_many_writes_what_separate_writes(tmp_path, monkeypatch, family):
    """[a file at the model's rate, one at 48 kHz, one at 96 kHz] in one pooled call: per file the bytes ``separate`` writes (the Demucs
    shift offsets are drawn in file order, so both runs start from one seed)."""
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    case = case_of(family, tmp_path)
    tag, cls, common, arch, wav, _ = case
    model_rate = common["sample_rate"]
    files = [rewritten(case, tmp_path, rate, name=f"song{rate}.wav")[0] for rate in (model_rate, 48000, 96000)]

    def run(out_sub, many):
        out_dir = os.path.join(common["output_dir"], out_sub)
        inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, asx_input_resample="device"), arch_config=arch)
        random.seed(4321)
        if many:
            results = inst.separate_many(files)
            assert inst.batch_errors == {}, inst.batch_errors
        else:
            results = []
            for f in files:
                results.append(inst.separate(f, None))
                inst.clear_file_specific_paths()
        blobs = []
        for names in results:
            assert names
            for n in names:
                with open(os.path.join(out_dir, n), "rb") as f:
                    blobs.append((n, f.read()))
        inst.clear_gpu_cache()
        return blobs

    one, many = run("one", False), run("many", True)
    assert [n for n, _ in one] == [n for n, _ in many]
    assert len({n for n, _ in one}) == len(one)
    for (n, a), (_, b) in zip(one, many):
        assert a == b, n


def _member(case, tmp, sub, **over):
    tag, cls, common, arch, _, _ = case
    return SC.plugin_class(cls)(common_config=dict(common, output_dir=os.path.join(common["output_dir"], sub), **over), arch_config=arch)


def test_ensemble_members_must_agree_and_take_the_file_on_the_device(tmp_path, monkeypatch):
    from audio_separator_amd.ensemble import EnsembleSeparator
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    mdx, mdxc = case_of("mdx", tmp_path), case_of("mdxc", tmp_path)
    with pytest.raises(ValueError, match="asx_input_resample"):
        EnsembleSeparator([_member(mdx, tmp_path, "e0", asx_input_resample="device"), _member(mdxc, tmp_path, "e0")])
    members = [_member(mdx, tmp_path, "e1", asx_input_resample="device"), _member(mdxc, tmp_path, "e1", asx_input_resample="device")]
    ens = EnsembleSeparator(members, algorithm="avg_wave")
    files = [rewritten(mdx, tmp_path, rate, name=f"song{rate}.wav")[0] for rate in (44100, 48000)]
    ens.output_dir = str(tmp_path / "ens")
    results = ens.separate_many(files)
    assert ens.batch_errors == {}, ens.batch_errors
    assert ens.last_paths_taken == ["device", "device"]
    assert all(results)
    from audio_separator_amd import audio_io
    frames = audio_io.wav_info(files[1])["frames"]
    for out in results[1]:
        info = audio_io.wav_info(os.path.join(ens.output_dir, out))
        assert info["samplerate"] == 44100 and info["frames"] == -(-frames * 147 // 160)
