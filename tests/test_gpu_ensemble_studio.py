"""Studio material through an ensemble on the MI355X: a 24-bit 48 kHz WAV, members that write with soundfile (``use_soundfile=True``,
the only writer that keeps the input's width) and take the file with ``asx_input_resample="device"``.

* ``EnsembleSeparator(intermediate="writer")`` keeps such members on the device path; the files are byte-identical to the literal flow
  (``via_files=True``: real intermediate files of the members' own formats, read back, combined on the host arrays);
* ``output_rate="input"`` writes the combined result at the file's rate with the file's frame count, the same bytes from ``separate``,
  ``separate_many`` and ``via_files=True``;
* the default ``EnsembleSeparator`` on the same members still takes the intermediate-file path.

soundfile is patched absent, as in tests/test_gpu_soundfile_writer.py: with it installed (and ``asx_output_encoder`` not "device")
libsndfile's float32 product makes the intermediates, which is not pinned here.  The inputs come from the helper of
tests/test_gpu_separate_rates.py (the golden clip repeated until the converted file is as long as the golden one)."""
import filecmp
import logging
import os
import random
import tempfile

import numpy as np
import pytest

from tests import flac_ref
from tests import separate_cases as SC
from tests.test_gpu_separate_rates import rewritten

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _environment(monkeypatch):
    from audio_separator_amd import audio_io
    real = audio_io._optional
    monkeypatch.setattr(audio_io, "_optional", lambda name: None if name == "soundfile" else real(name))
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    monkeypatch.setattr(random, "randint", lambda a, b: a + (b - a) // 3)      # the Demucs shift draws: the same on every path


def _member(case, **over):
    _, cls, common, arch, _, _ = case
    return SC.plugin_class(cls)(common_config=dict(common, asx_input_resample="device", **over), arch_config=arch)


@pytest.fixture(scope="module")
def studio(tmp_path_factory):
    """MDX + MDXC at 44.1 kHz, each with and without soundfile (and a FLAC-writing pair); the inputs: 24-bit 48 kHz, 24-bit 44.1 kHz,
    16-bit 48 kHz and a float64 one at the model's rate"""
    tmp = str(tmp_path_factory.mktemp("studio"))
    mdx, mdxc = SC.cases("mdx", tmp)[0], SC.cases("mdxc", tmp)[1]
    members = {"sf": [_member(mdx, use_soundfile=True), _member(mdxc, use_soundfile=True)],
               "mixed": [_member(mdx, use_soundfile=True), _member(mdxc)],
               "mixed_last": [_member(mdx), _member(mdxc, use_soundfile=True)],
               "plain": [_member(mdx), _member(mdxc)],
               "flac": [_member(mdx, use_soundfile=True, output_format="FLAC"), _member(mdxc, use_soundfile=True, output_format="FLAC")]}
    files = {"24_48": rewritten(mdx, tmp, 48000, "PCM_24", name="studio.wav"),
             "24_44": rewritten(mdx, tmp, 44100, "PCM_24", name="at_model_rate.wav"),
             "16_48": rewritten(mdx, tmp, 48000, "PCM_16", name="sixteen.wav"),
             "64_44": rewritten(mdx, tmp, 44100, "DOUBLE", name="double.wav")}
    return members, files


def _run(members, tmp_path, sub, paths, many=False, forbid_temp=False, monkeypatch=None, **kw):
    """One EnsembleSeparator over ``paths`` -> (ens, [[output file per stem] per path])"""
    import audio_separator_amd as A
    ens = A.EnsembleSeparator(members, kw.pop("algorithm", "avg_wave"), kw.pop("weights", None), **kw)
    ens.output_dir = str(tmp_path / sub)
    with monkeypatch.context() as mp:
        if forbid_temp:
            def no_temp_dir(*a, **k):
                raise AssertionError("the device path must not create a temporary directory")
            mp.setattr(tempfile, "mkdtemp", no_temp_dir)
        if many:
            out = ens.separate_many(paths)
            assert ens.batch_errors == {}, ens.batch_errors
        else:
            out = []
            for p in paths:
                out.append(ens.separate(p))
                ens.last_paths_taken.append(ens.last_path_taken)       # (separate keeps only the last one)
    return ens, out


def _same_files(got, want, got_dir, want_dir):
    assert [os.path.relpath(f, got_dir) for f in got] == [os.path.relpath(f, want_dir) for f in want] and got
    for a, b in zip(got, want):
        assert os.path.isfile(a) and os.path.isfile(b), (a, b)
        assert filecmp.cmp(a, b, shallow=False), os.path.basename(a)


@pytest.mark.parametrize("algorithm", ["avg_wave", "median_fft"])
def test_writer_intermediates_stay_on_the_device(studio, tmp_path, monkeypatch, algorithm):
    from audio_separator_amd import audio_io
    members, files = studio
    wav, frames = files["24_48"]
    weights = [1.0, 2.0] if algorithm == "avg_wave" else None
    by_files, want = _run(members["sf"], tmp_path, "files", [wav], monkeypatch=monkeypatch, algorithm=algorithm, weights=weights,
                          intermediate="writer", via_files=True)
    on_device, got = _run(members["sf"], tmp_path, "device", [wav], forbid_temp=True, monkeypatch=monkeypatch, algorithm=algorithm,
                          weights=weights, intermediate="writer")
    assert by_files.last_path_taken == "files" and on_device.last_path_taken == "device"
    _same_files(got[0], want[0], on_device.output_dir, by_files.output_dir)
    assert len(got[0]) == 2
    n_model = -(-frames * 147 // 160)
    for f in got[0]:
        info = audio_io.wav_info(f)
        assert (info["subtype"], info["samplerate"], info["frames"]) == ("PCM_24", 44100, n_model), f
        x, _ = audio_io.read_wav(f)
        assert np.abs(x).max() > 1e-4
    # members without soundfile (the truncating 16-bit intermediates, a 16-bit result widened to 24 bits) give other bytes
    _, narrow = _run(members["plain"], tmp_path, "plain", [wav], monkeypatch=monkeypatch, algorithm=algorithm, weights=weights)
    assert not filecmp.cmp(got[0][0], narrow[0][0], shallow=False)


def test_default_still_takes_the_file_path(studio, tmp_path, monkeypatch, caplog):
    members, files = studio
    wav, _ = files["24_48"]
    with caplog.at_level(logging.INFO):
        default, got = _run(members["sf"], tmp_path, "default", [wav], monkeypatch=monkeypatch)
    assert default.last_path_taken == "files" and "a member writes with soundfile" in caplog.text
    # ... which is the literal flow: the bytes of via_files=True, and of "writer" (its intermediates are those files)
    literal, want = _run(members["sf"], tmp_path, "literal", [wav], monkeypatch=monkeypatch, via_files=True)
    _same_files(got[0], want[0], default.output_dir, literal.output_dir)
    writer, same = _run(members["sf"], tmp_path, "writer", [wav], forbid_temp=True, monkeypatch=monkeypatch, intermediate="writer")
    _same_files(same[0], want[0], writer.output_dir, literal.output_dir)
    # without a soundfile member the default is the device path, as ever, and "writer" is that path bit for bit
    plain, a = _run(members["plain"], tmp_path, "plain", [wav], forbid_temp=True, monkeypatch=monkeypatch)
    plain_w, b = _run(members["plain"], tmp_path, "plain_w", [wav], forbid_temp=True, monkeypatch=monkeypatch, intermediate="writer")
    assert plain.last_path_taken == plain_w.last_path_taken == "device"
    _same_files(b[0], a[0], plain_w.output_dir, plain.output_dir)


@pytest.mark.parametrize("which", ["mixed", "mixed_last"])
def test_mixed_writers_in_one_ensemble(studio, tmp_path, monkeypatch, which):
    """one member with soundfile (PCM_24 intermediates), one without (the truncating 16-bit ones): each contributor its own round trip"""
    from audio_separator_amd import audio_io
    members, files = studio
    wav, _ = files["24_48"]
    by_files, want = _run(members[which], tmp_path, "files", [wav], monkeypatch=monkeypatch, algorithm="max_wave", intermediate="writer",
                          via_files=True)
    on_device, got = _run(members[which], tmp_path, "device", [wav], forbid_temp=True, monkeypatch=monkeypatch, algorithm="max_wave",
                          intermediate="writer")
    assert on_device.last_path_taken == "device"
    _same_files(got[0], want[0], on_device.output_dir, by_files.output_dir)
    # the last member writes the result: with soundfile at the input's width, without it pydub's way (24 bits of a 16-bit sample)
    assert audio_io.wav_info(got[0][0])["subtype"] == "PCM_24"


def test_output_rate_input(studio, tmp_path, monkeypatch):
    """[24-bit 48 kHz, 24-bit at the model's rate, 16-bit 48 kHz]: ``separate``, ``separate_many`` and the literal flow write the same
    bytes, at each file's own rate, frame count and width"""
    from audio_separator_amd import audio_io
    members, files = studio
    keys = ("24_48", "24_44", "16_48")
    paths = [files[k][0] for k in keys]
    kw = dict(intermediate="writer", output_rate="input")
    loop, one = _run(members["sf"], tmp_path, "loop", paths, forbid_temp=True, monkeypatch=monkeypatch, **kw)
    pooled, many = _run(members["sf"], tmp_path, "many", paths, many=True, forbid_temp=True, monkeypatch=monkeypatch, **kw)
    literal, lit = _run(members["sf"], tmp_path, "literal", paths, monkeypatch=monkeypatch, via_files=True, **kw)
    assert loop.last_paths_taken == pooled.last_paths_taken == ["device"] * 3 and literal.last_paths_taken == ["files"] * 3
    for k, a, b, c in zip(keys, one, many, lit):
        _same_files(b, a, pooled.output_dir, loop.output_dir)
        _same_files(c, a, literal.output_dir, loop.output_dir)
        rate, subtype = (48000 if k.endswith("48") else 44100), ("PCM_24" if k.startswith("24") else "PCM_16")
        for f in a:
            info = audio_io.wav_info(f)
            assert (info["samplerate"], info["frames"], info["subtype"]) == (rate, files[k][1], subtype), f
    # a file at the model's rate: nothing is converted -- the bytes written without the knob
    _, off = _run(members["sf"], tmp_path, "off", [paths[1]], forbid_temp=True, monkeypatch=monkeypatch, intermediate="writer")
    _same_files(off[0], one[1], str(tmp_path / "off"), loop.output_dir)
    # the members were not touched
    assert all(m.asx_output_rate == "model" and m._output_rate_override is None for m in members["sf"])
    # pydub's writer too: the default intermediates with the result at the file's rate, device path == literal flow
    dev, a = _run(members["plain"], tmp_path, "plain_dev", paths[:1], forbid_temp=True, monkeypatch=monkeypatch, output_rate="input")
    lit2, b = _run(members["plain"], tmp_path, "plain_lit", paths[:1], monkeypatch=monkeypatch, output_rate="input", via_files=True)
    assert dev.last_path_taken == "device"
    _same_files(a[0], b[0], dev.output_dir, lit2.output_dir)
    info = audio_io.wav_info(a[0][0])
    assert (info["samplerate"], info["frames"]) == (48000, files["24_48"][1])


def test_flac_output_holds_the_wav_runs_samples(studio, tmp_path, monkeypatch):
    from audio_separator_amd import audio_io
    members, files = studio
    wav, frames = files["24_48"]
    kw = dict(intermediate="writer", output_rate="input")
    as_wav, w = _run(members["sf"], tmp_path, "wav", [wav], forbid_temp=True, monkeypatch=monkeypatch, **kw)
    as_flac, f = _run(members["flac"], tmp_path, "flac", [wav], forbid_temp=True, monkeypatch=monkeypatch, **kw)
    assert as_flac.last_path_taken == "device" and len(f[0]) == len(w[0]) == 2
    for fw, ff in zip(w[0], f[0]):
        assert os.path.splitext(os.path.basename(fw))[0] == os.path.splitext(os.path.basename(ff))[0] and ff.endswith(".flac")
        with open(ff, "rb") as fh:
            info, pcm, _ = flac_ref.decode(fh.read())
        assert (info["samplerate"], info["bits_per_sample"], info["channels"], info["total_samples"]) == (48000, 24, 2, frames)
        samples, rate = audio_io.read_wav(fw)
        assert rate == 48000 and np.array_equal(pcm.T, np.rint(samples.astype(np.float64) * 8388608.0).astype(np.int64))
        assert (pcm & 0xff).any()                                   # true 24-bit samples


def test_a_double_input_goes_through_files(studio, tmp_path, monkeypatch, caplog):
    members, files = studio
    wav, _ = files["64_44"]
    with caplog.at_level(logging.INFO):
        ens, out = _run(members["sf"], tmp_path, "double", [wav, files["24_48"][0]], many=True, monkeypatch=monkeypatch, intermediate="writer")
    assert ens.last_paths_taken == ["files", "device"] and all(len(o) == 2 and all(os.path.isfile(f) for f in o) for o in out)
    assert "double.wav: ensemble through intermediate files" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO):
        ens, out = _run(members["sf"], tmp_path, "double_one", [wav], monkeypatch=monkeypatch, intermediate="writer")
    assert ens.last_path_taken == "files" and "double.wav: ensemble through intermediate files" in caplog.text and len(out[0]) == 2


def test_demucs_members(tmp_path, monkeypatch):
    """two HTDemucs members (8 kHz nets, four stems each) on a 24-bit 48 kHz file: "writer" and ``output_rate`` on the device path
    against the literal flow"""
    from audio_separator_amd import audio_io
    case = SC.cases("demucs", str(tmp_path))[0]
    members = [_member(case, use_soundfile=True), _member(case, use_soundfile=True)]
    wav, frames = rewritten(case, tmp_path, 48000, "PCM_24", name="studio8.wav")
    kw = dict(algorithm="avg_wave", weights=[2.0, 1.0], intermediate="writer", output_rate="input")
    random.seed(4321)
    by_files, want = _run(members, tmp_path, "files", [wav], monkeypatch=monkeypatch, via_files=True, **kw)
    random.seed(4321)
    on_device, got = _run(members, tmp_path, "device", [wav], forbid_temp=True, monkeypatch=monkeypatch, **kw)
    random.seed(4321)
    pooled, many = _run(members, tmp_path, "many", [wav], many=True, forbid_temp=True, monkeypatch=monkeypatch, **kw)
    assert on_device.last_path_taken == "device" and pooled.last_paths_taken == ["device"] and len(got[0]) == 4
    _same_files(got[0], want[0], on_device.output_dir, by_files.output_dir)
    _same_files(many[0], want[0], pooled.output_dir, by_files.output_dir)
    for f in got[0]:
        info = audio_io.wav_info(f)
        assert (info["samplerate"], info["frames"], info["subtype"]) == (48000, frames, "PCM_24"), f
