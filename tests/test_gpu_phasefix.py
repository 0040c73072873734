"""phasefix.PhaseFixSeparator on the device, with the tiny models and inputs of tests/separate_cases.py: the written file against the
float64 statement (tests/phasefix_ref.py) of the two members' ``stems_dev`` arrays after the target writer's rule; the device path against
``ASX_FILE_FASTPATH=0`` byte for byte (WAV, FLAC, one ``use_soundfile`` subtype, ``output_rate="input"`` on a 48 kHz input);
``separate_many`` against the loop; the paths taken.

Both members of a pair run at the input file's sample rate (a phase fix refuses members at different rates): ``sample_rate`` is the rate
the plugins read and write at, the tiny nets do not care.

Sample tolerance of the first test: the kernels are within 5e-6 of the float64 statement relative to its peak
(tests/test_gpu_phasefix_kernels.py), the writer scales a peak above 0.9 down to it and truncates x * 32767 to int16 -- 0.15 LSB of
error, so a sample may land on the other side of an integer: at most 1 LSB."""
import os
import random

import numpy as np
import pytest

from tests import phasefix_ref as R
from tests import separate_cases as SC
from tests.test_gpu_chain import blobs, golden_input, plugin, stem_name_of
from tests.test_gpu_separate_rates import rewritten

pytestmark = pytest.mark.gpu

# (target family, its stem, source family, its stem, compared with the statement?): every family once in either place; "s0" / "s1": the MDXC
# fixture's first / second instrument.  The stems of the last pair leave ambiguous bins (phasefix_ref.ambiguous_bins: 16 of them, and bins
# where the source is 2e-6 of its rms), where delta is +pi or -pi by the last bit and the float32 numpy statement itself is 2e-5 from the
# float64 one: there the comparison is not defined, and only the two paths are held against each other.
PAIRS = [("mdx", "Instrumental", "mdxc", "s1", True), ("demucs", "Bass", "vr", "Instrumental", True), ("mdxc", "s0", "mdx", "Vocals", False)]


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")


def stem_of(member, stem):
    if stem == "s1":
        return member.model_data["training"]["instruments"][1]
    return stem_name_of(member, stem)


def members(tmp, sub, f1, f2, rate, over1=None, over2=None):
    target, _ = plugin(f1, tmp, sub, rate, **(over1 or {}))
    source, _ = plugin(f2, tmp, sub, rate, **(over2 if over2 is not None else {k: v for k, v in (over1 or {}).items() if k == "asx_input_resample"}))
    return target, source


def fixer_of(tmp, sub, f1, s1, f2, s2, rate, over1=None, over2=None, **kw):
    from audio_separator_amd import PhaseFixSeparator
    target, source = members(tmp, sub, f1, f2, rate, over1, over2)
    return PhaseFixSeparator(target, source, (stem_of(target, s1), stem_of(source, s2)), **kw)


def input_of(f1, f2, tmp):
    path, rate = golden_input(f1, tmp)
    if "vr" in (f1, f2) and rate != 8000:
        # the VR fixture takes a device mix at its top band's rate, 8000 Hz: the same samples under that label
        path, rate = rewritten(SC.cases(f1, str(tmp / f"models_{f1}"))[0], tmp, 8000)[0], 8000
    return path, rate


def planar(entry):
    _, tensor, layout = entry
    a = tensor.detach().cpu().numpy()
    return np.ascontiguousarray(a if layout == "planar" else a.T)


def both_paths(tmp, monkeypatch, path, *args, **kw):
    """the same call on fresh members on the device path and under ASX_FILE_FASTPATH=0: (fixer, names) of each"""
    out = []
    for sub, env in (("dev", "1"), ("off", "0")):
        monkeypatch.setenv("ASX_FILE_FASTPATH", env)
        fixer = fixer_of(tmp, sub, *args, **kw)
        random.seed(4321)                                   # the Demucs shift offsets
        out.append((fixer, fixer.separate(path)))
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    (dev, got), (off, got_off) = out
    assert dev.last_path_taken == "device" and off.last_path_taken == "files" and got == got_off and len(got) == 1
    assert blobs(str(tmp / "dev"), got) == blobs(str(tmp / "off"), got)
    assert os.listdir(tmp / "dev") == got and os.listdir(tmp / "off") == got            # only the fixed stem is written
    return dev, off, got


@pytest.mark.parametrize("f1,s1,f2,s2,defined", PAIRS)
def test_file_is_the_statement_on_the_members_stems(tmp_path, monkeypatch, f1, s1, f2, s2, defined):
    from audio_separator_amd import audio_io, ensemble
    path, rate = input_of(f1, f2, tmp_path)
    probe_t, probe_s = members(tmp_path, "probe", f1, f2, rate)
    name_t, name_s = stem_of(probe_t, s1), stem_of(probe_s, s2)
    random.seed(4321)
    t = planar(next(e for e in probe_t.stems_dev(path) if e[0].lower() == name_t.lower()))
    s = planar(next(e for e in probe_s.stems_dev(path) if e[0].lower() == name_s.lower()))
    kw = {"low_hz": 200, "high_hz": 3000, "high_weight": 1.2, "hop": 256}
    dev, off, got = both_paths(tmp_path, monkeypatch, path, f1, s1.upper() if s1[0] != "s" else s1, f2, s2, rate, **kw)
    base = os.path.splitext(os.path.basename(path))[0]
    assert got == [f"{base}_({name_t})_phasefix_{ensemble.model_slugs(dev.model_filenames)}.wav"]
    weights = R.bin_weights(rate, 200, 3000, 0.0, 1.2)
    ambiguous = R.ambiguous_bins(t, s, weights, 256)
    print(f"PHASEFIX file {f1}+{f2}: {ambiguous} ambiguous bins")
    assert dev.target.audio_file_path is None and dev.source.audio_file_path is None     # the members' per-file state is reset
    if not defined:
        return
    assert ambiguous == 0, "the members' stems no longer leave the statement defined in every bin: choose other stems"
    ref = R.phase_fix(t, s, weights, 256).astype(np.float32).T
    peak = np.abs(ref).max()
    assert peak > 1e-3
    if peak > np.float32(0.9):
        ref = ref * (np.float32(0.9) / peak)
    want = (ref * 32767).astype(np.int16)
    data, file_rate = audio_io.read_wav(os.path.join(str(tmp_path / "dev"), got[0]))
    assert file_rate == rate and data.shape == (2, t.shape[1])                           # the target stem's length
    worst = int(np.abs(np.rint(data.T * 32768.0).astype(np.int64) - want).max())
    print(f"PHASEFIX file {f1}+{f2}: n={t.shape[1]} source n={s.shape[1]} worst int16 difference {worst}")
    assert worst <= 1


def test_custom_name(tmp_path):
    path, rate = input_of("mdx", "mdx", tmp_path)
    fixer = fixer_of(tmp_path, "out", "mdx", "Instrumental", "mdx", "Vocals", rate)
    assert fixer.separate(path, {"instrumental": "clean inst", "Vocals": "unused"}) == ["clean inst.wav"]
    assert os.listdir(tmp_path / "out") == ["clean inst.wav"] and fixer.last_path_taken == "device"


@pytest.mark.parametrize("subtype", ["PCM_16", "PCM_24"])
def test_flac_output(tmp_path, monkeypatch, subtype):
    from audio_separator_amd import audio_io
    path, _ = rewritten(SC.cases("mdx", str(tmp_path / "models_mdx"))[0], tmp_path, 44100, subtype)
    dev, _, got = both_paths(tmp_path, monkeypatch, path, "mdx", "Instrumental", "mdxc", "s1", 44100, over1={"output_format": "FLAC"}, over2={})
    assert got[0].endswith(".flac")
    assert audio_io.flac_stream(os.path.join(str(tmp_path / "dev"), got[0]))["bits_per_sample"] == (16 if subtype == "PCM_16" else 24)


def test_soundfile_output(tmp_path, monkeypatch):
    """``use_soundfile`` on the target: the result carries the input's own sample format, encoded on the device"""
    from audio_separator_amd import audio_io
    path, _ = rewritten(SC.cases("mdx", str(tmp_path / "models_mdx"))[0], tmp_path, 44100, "PCM_24")
    dev, _, got = both_paths(tmp_path, monkeypatch, path, "mdx", "Instrumental", "mdx", "Vocals", 44100,
                             over1={"use_soundfile": True, "asx_output_encoder": "device"}, over2={})
    assert dev.target.last_write_path == "wav_device_resident"
    assert audio_io.wav_info(os.path.join(str(tmp_path / "dev"), got[0]))["subtype"] == "PCM_24"


def test_output_rate_input_has_the_files_frame_count(tmp_path, monkeypatch):
    from audio_separator_amd import audio_io
    path, frames = rewritten(SC.cases("mdx", str(tmp_path / "models_mdx"))[0], tmp_path, 48000)
    dev, _, got = both_paths(tmp_path, monkeypatch, path, "mdx", "Instrumental", "mdx", "Vocals", 44100,
                             over1={"asx_input_resample": "device"}, output_rate="input")
    info = audio_io.wav_info(os.path.join(str(tmp_path / "dev"), got[0]))
    assert (info["samplerate"], info["frames"]) == (48000, frames)
    model = fixer_of(tmp_path, "model", "mdx", "Instrumental", "mdx", "Vocals", 44100, over1={"asx_input_resample": "device"})
    name = model.separate(path)[0]
    info = audio_io.wav_info(os.path.join(str(tmp_path / "model"), name))
    assert info["samplerate"] == 44100 and info["frames"] == -(-frames * 44100 // 48000)


def test_separate_many_is_the_loop(tmp_path):
    """Three files of different lengths and one unreadable path, two files per pooled phase fix: per file the bytes of ``separate``; the
    bad path fails alone."""
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
    loop = fixer_of(tmp_path, "loop", "mdx", "Instrumental", "mdx", "Vocals", rate)
    want = []
    for p in paths:
        try:
            want.append(loop.separate(p))
        except Exception:
            want.append([])
    many = fixer_of(tmp_path, "many", "mdx", "Instrumental", "mdx", "Vocals", rate, pool_files=3)
    n0 = many.target.engine.counter("phasefix_launches")
    got = many.separate_many(paths)
    assert many.target.engine.counter("phasefix_launches") - n0 == 4                    # two pooled calls: files 0, 1 (and the bad one), file 3
    assert got == want and got[2] == [] and all(len(g) == 1 for i, g in enumerate(got) if i != 2)
    assert sorted(many.batch_errors) == [2] and many.last_paths_taken == ["device", "device", "failed", "device"]
    assert many.last_path_taken == "device"
    for names in got:
        assert blobs(str(tmp_path / "many"), names) == blobs(str(tmp_path / "loop"), names)
