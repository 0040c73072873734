"""``EnsembleSeparator(intermediate="writer")`` and ``EnsembleSeparator(output_rate="input")`` without a device:

* the numpy restatement of the slot modes (tests/ensemble_slot_ref.py) against the real file round trip, audio_io.write_wav ->
  audio_io.read_wav, per subtype, and against hand values;
* the constructor's rules and ``_device_path_refusal``;
* with the member and engine doubles of tests/test_host_ensemble_batch.py: the per-contributor modes the pooled call is given for mixed
  members, the files that fall back to intermediate files, and the transient rate override the writer sees."""
import logging
import os
import types

import numpy as np
import pytest

from audio_separator_amd import audio_io
from audio_separator_amd.engine import Engine
from audio_separator_amd.ensemble import EnsembleSeparator
from tests import ensemble_slot_ref as SR
from tests.test_host_ensemble_batch import SILENT, FakeEngine, FakeMember, doubles  # noqa: F401  (doubles is a fixture)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _through_a_file(tmp_path, x, subtype, max_peak, min_peak):
    """``x`` planar [2, n] -> what audio_io.read_wav returns for the file audio_io.write_wav writes for the normalised stem"""
    y, peak = SR.normalize(x, max_peak, min_peak)
    path = str(tmp_path / f"{subtype}.wav")
    audio_io.write_wav(path, np.ascontiguousarray(y.T), 44100, subtype)
    back, rate = audio_io.read_wav(path)
    assert rate == 44100 and audio_io.wav_info(path)["subtype"] == subtype
    return back, peak


@pytest.mark.parametrize("subtype", SR.FILE_MODES)
@pytest.mark.parametrize("regime", [(1.7, 0.9, None), (0.2, 0.9, 0.5), (0.7, 0.9, 0.5), (1.0, 1.0, None)])
def test_restatement_is_the_file_round_trip(tmp_path, subtype, regime):
    amplitude, max_peak, min_peak = regime
    rng = np.random.default_rng(int(amplitude * 10) + len(subtype))
    x = (amplitude * rng.uniform(-1.0, 1.0, (2, 777))).astype(np.float32)
    x[0, 5], x[1, 9] = amplitude, -amplitude
    x[0, :4] = np.float32(0.5) * np.float32(amplitude), np.float32(-0.5) * np.float32(amplitude), 0.0, np.float32(amplitude) / 3
    want, peak = _through_a_file(tmp_path, x, subtype, max_peak, min_peak)
    got, peak_got = SR.round_trip(x, subtype, max_peak, min_peak)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert peak_got == peak


def test_hand_values():
    f32 = np.float32
    # exact .5 products: the only in-range float32 whose product with the odd 2^(b-1) - 1 is a half-integer is +-0.5 (k + .5 with k odd):
    # ties to even give +-2^(b-2), which read back as +-0.5 exactly; 1.5 would give an even k, but clips
    for bits, mode in ((16, "PCM_16"), (24, "PCM_24"), (32, "PCM_32")):
        full = (1 << (bits - 1)) - 1
        x = np.array([[0.5, -0.5, 1.0, -1.0, 0.0, 0.25]], f32).repeat(2, axis=0)
        q = SR.file_integers(x[0], bits)
        assert list(q) == [1 << (bits - 2), -(1 << (bits - 2)), full, -full, 0, int(np.rint(0.25 * full))]
        assert int(np.rint(2.5)) == 2 and int(np.rint(3.5)) == 4              # the rule itself: half to even
        back, peak = SR.round_trip(x, mode, 1.0, None)                        # peak 1.0 == max_peak: not scaled
        assert peak == f32(1.0) and back[0, 0] == f32(0.5) and back[0, 1] == f32(-0.5)
        # the peak lands on 2^(b-1) - 1, not on 2^(b-1): read back it is just below one
        assert back[0, 2] == f32(np.float64(full) / (1 << (bits - 1))) and back[0, 3] == -back[0, 2]
        # a peak of 2.0 against max_peak 1.0: the scale is exactly 0.5, the normalised peak exactly 1.0 -> 2^(b-1) - 1
        back2, peak2 = SR.round_trip(2 * x, mode, 1.0, None)
        assert peak2 == f32(1.0) and np.array_equal(back2, back)
        # negative full scale: only a value beyond -1 reaches -2^(b-1); beyond +1 clips to 2^(b-1) - 1
        wide = np.array([[-1.05, 1.05, -1.0 - 2.0 ** -20, 0.1]], f32).repeat(2, axis=0)
        qw = SR.file_integers(wide[0], bits)
        assert qw[0] == -(1 << (bits - 1)) and qw[1] == full
        back3, _ = SR.round_trip(wide, mode, 1.1, None)
        assert back3[0, 0] == f32(-1.0) and back3[0, 1] == back[0, 2]
        # the amplify branch: peak 0.25 below min_peak 0.5 -> scale exactly 2
        quiet = np.array([[0.25, -0.125, 0.0625, 0.0]], f32).repeat(2, axis=0)
        back4, peak4 = SR.round_trip(quiet, mode, 0.9, 0.5)
        assert peak4 == f32(0.5) and back4[0, 0] == f32(0.5) and back4[0, 1] == f32(np.float64(np.rint(-0.25 * full)) / (1 << (bits - 1)))
        back5, peak5 = SR.round_trip(quiet, mode, 0.9, None)                  # min_peak None: no amplification
        assert peak5 == f32(0.25) and back5[0, 0] == f32(np.float64(np.rint(0.25 * full)) / (1 << (bits - 1)))
    # the file PCM_16 rounds, the reference's pcm16 truncates: 0.7 * 32767 = 22936.9
    x = np.full((2, 1), 0.7, f32)
    assert SR.round_trip(x, "PCM_16", 0.9, None)[0][0, 0] == f32(22937 / 32768) and SR.round_trip(x, "pcm16", 0.9, None)[0][0, 0] == f32(22936 / 32768)
    # FLOAT: the normalised float itself; float32: the stem itself
    x = np.array([[1.8, -0.3]], f32).repeat(2, axis=0)
    scale = f32(0.9) / f32(1.8)
    back, peak = SR.round_trip(x, "FLOAT", 0.9, None)
    assert np.array_equal(back, x * scale) and peak == f32(1.8) * scale
    back, peak = SR.round_trip(x, "float32", 0.9, None)
    assert np.array_equal(back, x) and peak == f32(1.8)
    slot, _ = SR.slot_image(x, "PCM_24", 0.9, None, 5)
    assert slot.shape == (2, 5) and not slot[:, 2:].any() and slot[:, :2].all()


def test_engine_knows_the_modes_and_refuses_others():
    assert Engine.SLOT_MODES == {"pcm16": 0, "float32": 1, "PCM_16": 16, "PCM_24": 24, "PCM_32": 32, "FLOAT": 0x120}
    assert {Engine.SLOT_MODES[m] for m in SR.FILE_MODES} == {Engine.PCM_ENCODE_FORMATS[m] for m in SR.FILE_MODES}
    assert "asx_ensemble_batch_modes_dev" in __import__("audio_separator_amd.engine", fromlist=["SYMBOLS"]).SYMBOLS
    eng = object.__new__(Engine)                        # no library is reached: the names are judged before the call
    for call in (lambda: eng.ensemble_slot_dev(1, 4, "planar", 0.9, None, 1, 0, 4, mode="DOUBLE"),
                 lambda: eng.ensemble_slot_dev(1, 4, "planar", 0.9, None, 1, 0, 4, mode=16),
                 lambda: eng.ensemble_batch_dev([([(1, 4, "planar")], 1, 4)], "avg_wave", None, 0.9, None, mode="PCM_U8"),
                 lambda: eng.ensemble_batch_dev([([(1, 4, "planar"), (1, 4, "rows")], 1, 4)], "avg_wave", None, 0.9, None, modes=[["pcm16", "int24"]])):
        with pytest.raises(ValueError, match="unknown slot mode"):
            call()
    with pytest.raises(ValueError, match="one mode per contributor"):
        eng.ensemble_batch_dev([([(1, 4, "planar"), (1, 4, "rows")], 1, 4)], "avg_wave", None, 0.9, None, modes=[["pcm16"]])


# ---- constructor -----------------------------------------------------------------------------------------------------------------
def _stub(**over):
    m = types.SimpleNamespace(sample_rate=44100, normalization_threshold=0.9, amplification_threshold=0.0, use_soundfile=False,
                              output_dir="out", output_format="WAV", model_path="/m/a.onnx", model_name="a", logger=logging.getLogger("t"),
                              engine=None)
    m.stems_dev = lambda path: None
    for k, v in over.items():
        setattr(m, k, v)
    return m


def test_constructor_rules():
    ens = EnsembleSeparator([_stub(), _stub(use_soundfile=True)], intermediate="writer")
    assert ens.intermediate == "writer" and ens.output_rate == "model" and ens._device_path_refusal() is None
    assert "soundfile" in EnsembleSeparator([_stub(), _stub(use_soundfile=True)])._device_path_refusal()             # the default still refuses
    assert "soundfile" in EnsembleSeparator([_stub(use_soundfile=True)], intermediate="float32")._device_path_refusal()
    # "writer" with via_files is the literal flow; "float32" keeps its restriction
    assert EnsembleSeparator([_stub()], intermediate="writer", via_files=True)._device_path_refusal() == "via_files=True"
    with pytest.raises(ValueError, match="device path"):
        EnsembleSeparator([_stub()], intermediate="float32", via_files=True)
    with pytest.raises(ValueError, match="intermediate must be"):
        EnsembleSeparator([_stub()], intermediate="soundfile")
    # the other refusals of the device path stay under "writer"
    assert "output_format" in EnsembleSeparator([_stub(output_format="MP3")], intermediate="writer")._device_path_refusal()
    # output_rate
    assert EnsembleSeparator([_stub()], output_rate="input").output_rate == "input"
    for bad in ("file", "48000", None, 48000):
        with pytest.raises(ValueError, match="output_rate must be one of"):
            EnsembleSeparator([_stub()], output_rate=bad)
    # a member whose class refuses the knob itself (VRSeparator) refuses it for the ensemble too, saying why
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    assert VRSeparator._output_rate_refusal
    with pytest.raises(ValueError, match="output_rate='input' is not supported with a .* member: " + VRSeparator._output_rate_refusal[:20]):
        EnsembleSeparator([_stub(), _stub(_output_rate_refusal=VRSeparator._output_rate_refusal)], output_rate="input")
    EnsembleSeparator([_stub(), _stub(_output_rate_refusal=VRSeparator._output_rate_refusal)])                       # "model": no objection
    # members stay at "model": one at "input" is refused under either setting
    for kw in ({}, {"output_rate": "input"}):
        with pytest.raises(ValueError, match="asx_output_rate='input' is not supported in an ensemble"):
            EnsembleSeparator([_stub(), _stub(asx_output_rate="input")], **kw)


def test_slot_mode_of_a_member():
    on_device = lambda name: name.endswith((".wav", ".flac"))          # noqa: E731
    def sf(subtype, fmt="WAV", predicate=on_device):
        return _stub(use_soundfile=True, output_format=fmt, _output_subtype=lambda: subtype, _soundfile_on_device=predicate)
    ens = EnsembleSeparator([_stub()], intermediate="writer")
    assert ens._slot_mode(_stub()) == ("pcm16", None)
    for subtype in SR.FILE_MODES:
        assert ens._slot_mode(sf(subtype)) == (subtype, None)
    assert ens._slot_mode(sf("PCM_24", "FLAC")) == ("PCM_24", None) and ens._slot_mode(sf("PCM_16", "flac")) == ("PCM_16", None)
    for member, text in ((sf("DOUBLE"), "DOUBLE"), (sf("PCM_U8"), "PCM_U8"), (sf("PCM_32", "FLAC"), "FLAC holds no PCM_32"),
                         (sf("FLOAT", "flac"), "FLAC holds no FLOAT"), (sf("PCM_24", predicate=lambda name: False), "on the host")):
        mode, why = ens._slot_mode(member)
        assert mode is None and text in why
    # the other settings: one mode for everybody, the member is not asked
    assert EnsembleSeparator([_stub()])._slot_mode(sf("DOUBLE")) == ("pcm16", None)
    assert EnsembleSeparator([_stub()], intermediate="float32")._slot_mode(sf("DOUBLE")) == ("float32", None)


# ---- the pooled path over doubles --------------------------------------------------------------------------------------------------
class ModesEngine(FakeEngine):
    """records the mode arguments of every pooled call"""

    def __init__(self, registry):
        super().__init__(registry)
        self.how = []

    def ensemble_batch_dev(self, jobs, algorithm, weights, max_peak, min_peak, silent_below=SILENT, stream=0, **how):
        self.how.append(how)
        return super().ensemble_batch_dev(jobs, algorithm, weights, max_peak, min_peak, silent_below)


class WriterMember(FakeMember):
    """a member with a writer: the subtype and rate of each file come back with ``_restore_file``; ``write_audio`` records the override"""
    _output_rate_override = None
    SUBTYPES = {"float_song": "FLOAT", "double_song": "DOUBLE"}

    def __init__(self, *a, soundfile=False, float_as=None, **kw):
        super().__init__(*a, **kw)
        self.use_soundfile, self.float_as, self.overrides = soundfile, float_as, []

    def stems_dev_many(self, paths):
        stems, states = super().stems_dev_many(paths)
        for state in states:
            if state is not None:
                base = state["audio_file_base"]
                state["input_subtype"] = self.SUBTYPES.get(base, "PCM_24")
                state["_file_rate"], state["_file_frames"] = (48000, 1000 + len(base)) if base != "plain" else (44100, 900)
        return stems, states

    def _restore_file(self, state):
        super()._restore_file(state)
        self.input_subtype, self._file_rate, self._file_frames = state["input_subtype"], state["_file_rate"], state["_file_frames"]

    def _reset_file_state(self):
        super()._reset_file_state()
        self.input_subtype = self._file_rate = self._file_frames = None

    def _output_subtype(self):
        return self.float_as if self.float_as and self.input_subtype == "FLOAT" else self.input_subtype

    def _soundfile_on_device(self, name):
        return True

    def write_audio(self, path, source):
        self.overrides.append(self._output_rate_override)
        super().write_audio(path, source)


def _pool(doubles, **kw):
    ENS, registry, _ = doubles
    engine = ModesEngine(registry)
    a = WriterMember("model_a", ["Vocals", "Instrumental"], registry, engine, soundfile=True, float_as="PCM_32")
    b = WriterMember("model_b", ["Vocals"], registry, engine, soundfile=False)
    c = WriterMember("model_c", ["Vocals", "Instrumental"], registry, engine, soundfile=True)
    ens = ENS.EnsembleSeparator([a, b, c], "avg_wave", **kw)
    ens._free_hbm = lambda: None
    return ens, engine, (a, b, c)


def test_pooled_call_gets_each_contributors_mode(doubles, monkeypatch, caplog):
    ens, engine, (a, b, c) = _pool(doubles, intermediate="writer")
    via = []
    monkeypatch.setattr(ens, "_separate_via_files", lambda path, custom: via.append(path) or ["files"])
    paths = ["/p/song.wav", "/p/float_song.wav", "/p/double_song.wav"]
    with caplog.at_level(logging.INFO):
        got = ens.separate_many(paths)
    # jobs: (song, Vocals) a + b + c, (song, Instrumental) a + c, then float_song's: a VR-like member writes the FLOAT input as PCM_32
    assert engine.how == [{"modes": [["PCM_24", "pcm16", "PCM_24"], ["PCM_24", "PCM_24"], ["PCM_32", "pcm16", "FLOAT"], ["PCM_32", "FLOAT"]]}]
    assert engine.calls == [[3, 2, 3, 2]]
    # the DOUBLE file goes through intermediate files, alone, with the log line
    assert ens.last_paths_taken == ["device", "device", "files"] and via == [paths[2]] and got[2] == ["files"]
    assert "double_song.wav: ensemble through intermediate files (member 0, model_a, writes DOUBLE intermediates" in caplog.text
    # no rate override under output_rate = "model"
    assert c.overrides == [None] * 4 and c._output_rate_override is None


def test_other_intermediates_pass_one_mode_as_before(doubles):
    for kw, how in (({}, {"mode": "pcm16"}), ({"intermediate": "float32"}, {"mode": "float32"})):
        ens, engine, members = _pool(doubles, **kw)
        for m in members:
            m.use_soundfile = False
        ens.separate_many(["/p/song.wav"])
        assert engine.how == [how]


def test_rate_override_is_transient(doubles):
    ens, engine, (a, b, c) = _pool(doubles, intermediate="writer", output_rate="input")
    c.asx_output_rate = "model"
    got = ens.separate_many(["/p/song.wav", "/p/plain.wav"])
    assert ens.last_paths_taken == ["device", "device"] and all(len(g) == 2 for g in got)
    # the writer (the last member) sees this file's (rate, frames) during each write_audio call and nothing afterwards
    assert c.overrides == [(48000, 1004), (48000, 1004), (44100, 900), (44100, 900)]
    assert c._output_rate_override is None and c.asx_output_rate == "model" and a.overrides == [] and b.overrides == []
    # an exception in the writer does not leave the override behind
    def boom(path, source):
        raise RuntimeError("disk full")
    c.write_audio = boom
    with pytest.raises(RuntimeError):
        ens._write("/p/song.wav", "Vocals", np.zeros((4, 2), np.float32), None, (48000, 4))
    assert c._output_rate_override is None


def test_writer_hook_in_common_separator():
    """``_output_rate_target`` under the override: the knob stays "model", the override's rate and frames decide"""
    from audio_separator_amd.common_separator import CommonSeparator
    plans = []
    eng = types.SimpleNamespace(resample_rational_plan=lambda a, b, n: plans.append((a, b, n)) or (n, 0))
    w = object.__new__(CommonSeparator)
    w.asx_output_rate, w.engine, w.sample_rate, w.audio_file_path = "model", eng, 44100, "/p/x.wav"
    w._file_rate, w._file_frames, w._out_rate_warned = 96000, 7, False
    w.logger = logging.getLogger("hook")
    assert w._output_rate_override is None and w._output_rate_target() is None
    w._output_rate_override = (48000, 1234)
    assert w._output_rate_target() == (48000, 1234) and plans == [(44100, 48000, 1)]
    w._output_rate_override = (44100, 1234)
    assert w._output_rate_target() is None                      # a file at the model's rate: nothing is converted
    w._output_rate_override = (None, None)
    assert w._output_rate_target() is None and w._out_rate_warned          # unknown rate: one warning, the model's rate
    w._output_rate_override = None
    assert w._output_rate_target() is None
