"""phasefix.PhaseFixSeparator without a GPU: every refusal of the constructor, the names, ``custom_output_names``, the length rule, the
paths taken and the fail-alone rule of ``separate_many``, the C view of the new struct and the argument checks that need no device.

The members are real ``CommonSeparator`` subclasses (naming, writer, per-file state are the product's) over a subclass of the engine
double of tests/fake_engine.py whose ``phase_fix`` is the float64 statement of tests/phasefix_ref.py; the device path itself is
tests/test_gpu_phasefix.py's."""
from __future__ import annotations

import ctypes as C
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import phasefix_ref as R
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 8000


# ---- doubles -----------------------------------------------------------------------------------------------------------------------
class PhaseEngine(OracleEngine):
    """the writer's arithmetic of the double plus the phase fix as its float64 statement, rounded to float32"""
    calls = []

    def __init__(self, device=0):
        super().__init__(None, device)

    def phase_fix(self, target, source, bin_weights, hop=512):
        PhaseEngine.calls.append((target.shape, source.shape, hop))
        w = np.asarray(bin_weights)
        assert w.dtype == np.float32 and w.shape == (R.NB,)
        return np.ascontiguousarray(R.phase_fix(target.T, source.T, w, hop).T.astype(np.float32))


def make_member(name, out_dir, stems, shift=0, cut=0, min_len=0, device=0, dev_stems=None, **over):
    """A plugin whose stem ``s`` is ``gain_s`` x the mix delayed by ``shift`` samples and shortened by ``cut``; ``stems``: [(stem name, gain)]
    in the order written."""
    from audio_separator_amd.common_separator import CommonSeparator

    class StubMember(CommonSeparator):
        def _stems(self, mix):
            x = np.roll(mix, self.shift, axis=1)[:, : mix.shape[1] - self.cut]
            return {n: np.ascontiguousarray((np.float32(g) * x).T) for n, g in self.stems}

        def separate(self, audio_file_path, custom_output_names=None):
            self._begin_file(audio_file_path)
            _, host_mix = self._load_mix(audio_file_path)
            if host_mix.shape[1] < self.min_len:
                raise ValueError(f"input too short: {host_mix.shape[1]} samples")
            self.demixes += 1
            files = []
            made = self._stems(host_mix)
            for n, _ in self.stems:
                if self._wanted(n):
                    self._emit_stem(n, made[n], custom_output_names, files)
            return files

    config = {"logger": logging.getLogger("phasefix_test"), "model_name": name, "output_dir": str(out_dir), "output_format": "WAV",
              "normalization_threshold": 0.9, "amplification_threshold": 0.0, "sample_rate": RATE, "use_soundfile": False,
              "torch_device": f"cuda:{device}", "model_data": {}}
    config.update(over)
    member = StubMember(config)
    member.engine = PhaseEngine(device)
    member.stems, member.shift, member.cut, member.min_len, member.demixes = list(stems), shift, cut, min_len, 0
    member.primary_stem_name, member.secondary_stem_name = stems[0][0], stems[1][0]
    if dev_stems is not None:
        member.stems_dev = dev_stems
    return member


def write_input(path, n, seed, scale=0.5):
    from audio_separator_amd import audio_io
    rng = np.random.default_rng(seed)
    x = (scale * rng.uniform(-1, 1, (n, 2))).astype(np.float32)
    audio_io.write_wav(str(path), x, RATE, "PCM_16")
    return str(path), x


FULL = [("Vocals", 0.3), ("Instrumental", 0.9)]
CLEAN = [("Vocals", 0.5), ("Other", 0.7)]


def pair(tmp_path, sub="out", **over):
    return (make_member("full_model", tmp_path / sub, FULL, **over.get("target", {})),
            make_member("clean_model", tmp_path / sub, CLEAN, shift=3, **over.get("source", {})))


# ---- construction --------------------------------------------------------------------------------------------------------------------
def test_construction_refusals(tmp_path):
    from audio_separator_amd import PhaseFixSeparator as P
    t = lambda **o: make_member("a", tmp_path, FULL, **o)      # noqa: E731
    s = lambda **o: make_member("b", tmp_path, CLEAN, **o)     # noqa: E731
    stem = ("Instrumental", "Other")
    a = t()
    with pytest.raises(ValueError, match="two plugin instances"):
        P(a, a, stem)
    with pytest.raises(ValueError, match=r"the members differ in sample_rate \(8000 and 44100\)"):
        P(t(), s(sample_rate=44100), stem)
    with pytest.raises(ValueError, match=r"the two engines are on different devices \(0 and 1\)"):
        P(t(), s(device=1), stem)
    with pytest.raises(ValueError, match=r"the members differ in asx_input_resample: \['device', 'host'\]"):
        P(t(asx_input_resample="device"), s(), stem)
    for which, kw in (("target", ({"asx_output_rate": "input"}, {})), ("source", ({}, {"asx_output_rate": "input"}))):
        with pytest.raises(ValueError, match=rf"asx_output_rate='input' on the {which} is not supported in a phase fix"):
            P(t(**kw[0]), s(**kw[1]), stem)
    with pytest.raises(ValueError, match=r"target.output_single_stem is 'Vocals', so the stem 'Instrumental' would never be produced"):
        P(t(output_single_stem="Vocals"), s(), stem)
    with pytest.raises(ValueError, match=r"source.output_single_stem is 'Vocals', so the stem 'Other' would never be produced"):
        P(t(), s(output_single_stem="Vocals"), stem)
    P(t(output_single_stem="instrumental"), s(output_single_stem="OTHER"), stem)          # compared without case
    for hop in (0, 128, 500, 2048, "512"):
        with pytest.raises(ValueError, match=r"hop must be one of \(256, 512, 1024\)"):
            P(t(), s(), stem, hop=hop)
    with pytest.raises(ValueError, match=r"low_hz \(600\) is above high_hz \(500\)"):
        P(t(), s(), stem, low_hz=600, high_hz=500)
    P(t(), s(), stem, low_hz=500, high_hz=500)
    for kw in ({"low_weight": float("nan")}, {"high_weight": float("inf")}, {"high_weight": -float("inf")}, {"low_weight": 1e39}):
        with pytest.raises(ValueError, match="the weights must be finite"):
            P(t(), s(), stem, **kw)
    P(t(), s(), stem, low_weight=-3.5, high_weight=17.0)                                  # any finite weights
    with pytest.raises(ValueError, match="output_rate must be one of"):
        P(t(), s(), stem, output_rate="file")
    with pytest.raises(ValueError, match="pool_files must be at least 1"):
        P(t(), s(), stem, pool_files=0)
    with pytest.raises(ValueError, match="stem is"):
        P(t(), s(), ("a", "b", "c"))
    refusing = s()
    type(refusing)._output_rate_refusal = "its stems do not line up with the file"
    with pytest.raises(ValueError, match=r"output_rate='input' is not supported with a StubMember member: its stems do not line up"):
        P(t(), refusing, stem, output_rate="input")
    P(t(), refusing, stem)
    d = P(t(), s(), stem)                                                                 # the defaults and where they land
    assert (d.low_hz, d.high_hz, d.low_weight, d.high_weight, d.hop, d.output_rate, d.pool_files) == (500, 5000, 0.0, 0.8, 512, "model", None)
    assert np.array_equal(d.weights, R.bin_weights(RATE)) and d.weights.dtype == np.float32
    assert P(t(), s()).stem == ("Instrumental", "Instrumental") and P(t(), s(), "Vocals").stem == ("Vocals", "Vocals")


# ---- one file --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("custom", [None, {"instrumental": "fixed inst", "Vocals": "unused"}])
def test_host_path_names_length_and_samples(tmp_path, custom, caplog):
    from audio_separator_amd import PhaseFixSeparator, audio_io
    path, x = write_input(tmp_path / "song_(live).wav", 3000, 1)
    target, source = pair(tmp_path, source={"cut": 700})
    fixer = PhaseFixSeparator(target, source, ("instrumental", "OTHER"), low_hz=300, high_hz=2000, high_weight=1.0, hop=256)
    PhaseEngine.calls.clear()
    with caplog.at_level(logging.INFO, logger="phasefix_test"):
        got = fixer.separate(path, custom)
    want_name = "fixed inst.wav" if custom else "song_(live)_(Instrumental)_phasefix_full_model_clean_model.wav"
    assert got == [want_name] and fixer.last_path_taken == "files"
    assert PhaseEngine.calls == [((3000, 2), (2300, 2), 256)]                  # the stems as the members hand them to their writers
    assert os.listdir(tmp_path / "out") == [want_name]                        # only the fixed stem is written; the members' files are gone
    assert sum("phase fix through the members' host arrays (" in r.getMessage() for r in caplog.records) == 1     # one line saying why
    assert target.demixes == 1 and source.demixes == 1 and target._writer_tap is None and source._writer_tap is None
    assert target.output_dir == str(tmp_path / "out") and source.output_dir == str(tmp_path / "out")
    # the file: the float64 statement on the members' stems, through the target writer's rule (peak above 0.9 -> scaled, int16 truncation)
    mix = audio_io.load(path, mono=False, sr=RATE)[0]
    t = np.float32(0.9) * mix
    s = (np.float32(0.7) * np.roll(mix, 3, axis=1))[:, :2300]
    ref = R.phase_fix(t, s, R.bin_weights(RATE, 300, 2000, 0.0, 1.0), 256).astype(np.float32).T
    pcm, _ = target.engine.pcm16(ref, 0.9, 0.0)
    data, rate = audio_io.read_wav(str(tmp_path / "out" / want_name))
    assert rate == RATE and data.shape == (2, 3000)                            # the target stem's length
    assert np.array_equal(np.round(data.T * 32768).astype(np.int16), pcm)


def test_a_member_that_keeps_nothing_on_the_device_takes_the_host_path(tmp_path, monkeypatch, caplog):
    from audio_separator_amd import phasefix as PF
    monkeypatch.setattr(PF.PhaseFixSeparator, "_device_path_refusal", lambda self: None)     # as on a machine with a GPU
    path, _ = write_input(tmp_path / "song.wav", 1500, 2)
    asked = []
    target, source = pair(tmp_path, target={"dev_stems": lambda p: asked.append(p)})          # (returns None: the host decoder's file)
    fixer = PF.PhaseFixSeparator(target, source, ("Instrumental", "Other"))
    with caplog.at_level(logging.INFO, logger="phasefix_test"):
        got = fixer.separate(path)
    assert asked == [path] and fixer.last_path_taken == "files" and got == ["song_(Instrumental)_phasefix_full_model_clean_model.wav"]
    assert [r.getMessage() for r in caplog.records if "phase fix through" in r.getMessage()] == [
        f"{path}: phase fix through the members' host arrays (full_model needs the host decoder)"]
    lit_t, lit_s = pair(tmp_path, "lit")
    monkeypatch.undo()
    assert PF.PhaseFixSeparator(lit_t, lit_s, ("Instrumental", "Other")).separate(path) == got
    assert open(tmp_path / "out" / got[0], "rb").read() == open(tmp_path / "lit" / got[0], "rb").read()


def test_env_switch_and_unknown_stem(tmp_path, monkeypatch):
    from audio_separator_amd import PhaseFixSeparator
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    target, source = pair(tmp_path)
    assert PhaseFixSeparator(target, source, ("Instrumental", "Other"))._device_path_refusal() == "ASX_FILE_FASTPATH=0"
    path, _ = write_input(tmp_path / "song.wav", 900, 3)
    with pytest.raises(ValueError, match=r"'Drums' is not a stem clean_model produces for .*song.wav: it has \['Vocals', 'Other'\]"):
        PhaseFixSeparator(target, source, ("Instrumental", "Drums")).separate(path)
    assert not os.path.exists(tmp_path / "out") or os.listdir(tmp_path / "out") == []


def test_single_stem_members_write_nothing_else(tmp_path):
    from audio_separator_amd import PhaseFixSeparator
    path, _ = write_input(tmp_path / "song.wav", 1200, 4)
    target, source = pair(tmp_path, target={"output_single_stem": "Instrumental"}, source={"output_single_stem": "other"})
    got = PhaseFixSeparator(target, source, ("Instrumental", "Other")).separate(path)
    both_t, both_s = pair(tmp_path, "both")
    assert PhaseFixSeparator(both_t, both_s, ("Instrumental", "Other")).separate(path) == got
    assert open(tmp_path / "out" / got[0], "rb").read() == open(tmp_path / "both" / got[0], "rb").read()


# ---- separate_many -------------------------------------------------------------------------------------------------------------------
def test_separate_many_fails_alone(tmp_path):
    from audio_separator_amd import PhaseFixSeparator
    paths = [write_input(tmp_path / "one.wav", 1500, 5)[0], str(tmp_path / "missing.wav"), write_input(tmp_path / "short.wav", 300, 6)[0],
             write_input(tmp_path / "four.wav", 1100, 7)[0]]
    loop_t, loop_s = pair(tmp_path, "loop", source={"min_len": 500})
    loop = PhaseFixSeparator(loop_t, loop_s, ("Instrumental", "Other"))
    want = {i: loop.separate(paths[i]) for i in (0, 3)}
    target, source = pair(tmp_path, source={"min_len": 500})
    fixer = PhaseFixSeparator(target, source, ("Instrumental", "Other"), pool_files=2)
    got = fixer.separate_many(paths)
    assert got[0] == want[0] and got[3] == want[3] and got[1] == [] and got[2] == []
    assert sorted(fixer.batch_errors) == [1, 2] and "too short" in str(fixer.batch_errors[2])
    assert fixer.last_paths_taken == ["files", "failed", "failed", "files"] and fixer.last_path_taken == "files"
    for i in (0, 3):
        assert open(tmp_path / "out" / got[i][0], "rb").read() == open(tmp_path / "loop" / got[i][0], "rb").read()
    assert sorted(os.listdir(tmp_path / "out")) == sorted(got[0] + got[3])
    assert fixer.separate_many([]) == [] and fixer.batch_errors == {} and fixer.last_paths_taken == []


def test_pool_rule_is_the_ensembles(tmp_path):
    """one helper, not a copy: the runs of a phase fix are ensemble.pooled_runs', and EnsembleSeparator._runs is that helper too"""
    from audio_separator_amd import ensemble as ENS
    paths = [write_input(tmp_path / f"{i}.wav", n, i)[0] for i, n in enumerate((1000, 1000, 3000, 500))]
    assert ENS.pooled_runs(paths, 3, lambda: None, 16, 0.4) == [[0, 1, 2], [3]]
    assert ENS.pooled_runs(paths, None, lambda: None, 16, 0.4) == [[0, 1, 2, 3]]
    assert ENS.pooled_runs(paths, None, lambda: 2000.5 * 16 / 0.4, 16, 0.4) == [[0, 1], [2], [3]]
    target, source = pair(tmp_path)
    ens = ENS.EnsembleSeparator([target, source])
    ens._free_hbm = lambda: 2000.5 * 32 / 0.4
    assert ens._runs(paths) == [[0, 1], [2], [3]] and ENS.stems_per_file(target) == 2


# ---- the C view ------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_device_free_refusals(tmp_path):
    from audio_separator_amd import engine as E
    assert C.sizeof(E._PhaseJob) == 56 and E._PhaseJob.n_samples.offset == 24 and E._PhaseJob.out_layout.offset == 48
    assert E.PHASE_BINS == 1025 and E.PHASE_HOPS == (256, 512, 1024)
    gcc = shutil.which("gcc")
    if gcc:
        src = '#include <stdio.h>\n#include <stddef.h>\n#include "asx.h"\nint main(void) { printf("%zu %zu %d\\n", sizeof(asx_phase_job), ' \
              'offsetof(asx_phase_job, out_layout), ASX_PHASE_BINS); return 0; }\n'
        (tmp_path / "s.c").write_text(src)
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
        assert subprocess.run([str(tmp_path / "s")], check=True, capture_output=True, text=True).stdout.split() == ["56", "48", "1025"]
    import __graft_entry__ as entry
    entry.build()
    lib = E.load_library()
    w = (C.c_float * 1025)()
    job = E._PhaseJob(None, None, None, 10, 0, 0, 0, 0, 0)
    # the arguments are judged before the engine: the refusals can be told apart without a device
    assert lib.asx_phase_fix_batch_dev(None, C.byref(job), 1, w, 300, None) != 0 and b"hop 300" in lib.asx_last_error()
    assert lib.asx_phase_fix_batch_dev(None, C.byref(job), 1, w, 512, None) != 0 and b"job 0: the target is null" in lib.asx_last_error()
    assert lib.asx_phase_fix_batch_dev(None, None, 1, w, 512, None) != 0 and b"bad argument" in lib.asx_last_error()
    assert lib.asx_phase_fix_batch_dev(None, None, 0, None, 512, None) != 0 and b"null bin weights" in lib.asx_last_error()
    w[7] = float("nan")
    assert lib.asx_phase_fix_batch_dev(None, None, 0, w, 512, None) != 0 and b"weight of bin 7 is not finite" in lib.asx_last_error()
    w[7] = 0.0
    assert lib.asx_phase_fix_batch_dev(None, None, 0, w, 512, None) != 0 and b"null engine" in lib.asx_last_error()
    assert lib.asx_phase_fix_dev(None, None, w, 512, None) != 0 and b"null job" in lib.asx_last_error()
    assert lib.asx_phase_fix(None, None, 0, 10, None, 0, 0, w, 512, None, 0) != 0 and lib.asx_last_error()
