"""workflow.ChainSeparator without a GPU: the refusals, the literal flow's order / names / bytes, the fail-alone rule of
``separate_many``, the door of CommonSeparator, the mix-down rule against exact sums, and the C view of the two new structs.

The stages are real ``CommonSeparator`` subclasses (naming, writer, per-file state and the pooled shell are the product's) over a
numpy engine double of this file; the device path itself is tests/test_gpu_chain.py's."""
from __future__ import annotations

import ctypes as C
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.mixdown_ref import mixdown_exact, mixdown_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 8000


# ---- doubles -----------------------------------------------------------------------------------------------------------------------
class HostEngine:
    """the writer's arithmetic on the host: spec_utils.normalize and the truncating int16 pass"""

    def __init__(self, device=0):
        self.device = device

    @staticmethod
    def normalize(wave, max_peak=1.0, min_peak=None):
        peak = np.float32(np.abs(wave).max()) if wave.size else np.float32(0)
        if peak > np.float32(max_peak):
            wave *= np.float32(max_peak) / peak
        elif min_peak is not None and peak < np.float32(min_peak):
            wave *= np.float32(min_peak) / peak
        return wave

    def pcm16(self, stem, max_peak=1.0, min_peak=None):
        a = self.normalize(np.array(stem, np.float32, copy=True), max_peak, min_peak)
        return (a * 32767).astype(np.int16), float(np.abs(a).max()) if a.size else 0.0


def make_stage(name, out_dir, stems, min_len=0, late_stems=False, device=0, **over):
    """A plugin whose stem ``s`` is ``gain_s * mix``; ``stems``: [(stem name, gain)] in the order written."""
    from audio_separator_amd.common_separator import CommonSeparator

    class StubStage(CommonSeparator):
        def _stems(self, mix):
            return {n: np.ascontiguousarray((np.float32(g) * mix).T) for n, g in self.stems}

        def _check_loaded(self, dev_mix, host_mix):
            n = (host_mix if host_mix is not None else dev_mix).shape[1]
            if n < self.min_len:
                raise ValueError(f"input too short: {n} samples")

        def _emit_file(self, stems, on_device, custom_output_names):
            files = []
            self.primary_source, self.secondary_source = stems[self.stems[0][0]], stems[self.stems[1][0]]
            for n, _ in self.stems:
                if self._wanted(n):
                    self._emit_stem(n, stems[n], custom_output_names, files)
            return files

        def separate(self, audio_file_path, custom_output_names=None):
            self._begin_file(audio_file_path)
            dev_mix, host_mix = self._load_mix(audio_file_path)
            self._check_loaded(dev_mix, host_mix)
            self.demixes += 1
            return self._emit_file(self._stems(host_mix), False, custom_output_names)

        separate_many = CommonSeparator._separate_many

        def _pooled_stems(self, mixes):
            self.pooled_calls += 1
            return [self._stems(h) for _, h in mixes]

    config = {"logger": logging.getLogger("chain_test"), "model_name": name, "output_dir": str(out_dir), "output_format": "WAV",
              "normalization_threshold": 0.9, "amplification_threshold": 0.0, "sample_rate": RATE, "use_soundfile": False,
              "torch_device": f"cuda:{device}", "model_data": {}}
    config.update(over)
    stage = StubStage(config)
    stage.engine = HostEngine(device)
    stage.stems, stage.min_len, stage.demixes, stage.pooled_calls = list(stems), min_len, 0, 0
    stage.primary_stem_name, stage.secondary_stem_name = stems[0][0], stems[1][0]
    if late_stems:
        stage.demucs_source_map = {}          # (what marks a plugin whose stems are known only after its model is loaded)
    return stage


def write_input(path, n, seed, scale=0.5):
    from audio_separator_amd import audio_io
    rng = np.random.default_rng(seed)
    x = (scale * rng.uniform(-1, 1, (n, 2))).astype(np.float32)
    audio_io.write_wav(str(path), x, RATE, "PCM_16")
    return str(path)


FIRST = [("Vocals", 1.7), ("Instrumental", 0.6)]          # 1.7 * 0.5 peaks near 0.85 .. see test_weight_rule for a stem above 0.9
THEN = [("Lead", 0.5), ("Backing", 0.25)]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def literal(first, then, path, stem_name, custom=None):
    a = first.separate(path, custom)
    stem_file = first.get_stem_output_path(stem_name, custom)
    b = then.separate(os.path.join(first.output_dir, stem_file), custom)
    return a + b


# ---- construction --------------------------------------------------------------------------------------------------------------------
def test_construction_refusals(tmp_path):
    from audio_separator_amd.workflow import ChainSeparator
    mk = lambda n, **o: make_stage(n, tmp_path, FIRST if n == "a" else THEN, **o)  # noqa: E731
    with pytest.raises(ValueError, match=r"handoff must be one of \('file', 'float'\), not 'pcm'"):
        ChainSeparator(mk("a"), mk("b"), "Vocals", handoff="pcm")
    with pytest.raises(ValueError, match=r"the stages differ in sample_rate \(8000 and 44100\)"):
        ChainSeparator(mk("a"), mk("b", sample_rate=44100), "Vocals")
    for which, kw in (("first", ({"asx_output_rate": "input"}, {})), ("then", ({}, {"asx_output_rate": "input"}))):
        with pytest.raises(ValueError, match=rf"asx_output_rate='input' on the {which} stage is not supported in a chain.*out of scope"):
            ChainSeparator(mk("a", **kw[0]), mk("b", **kw[1]), "Vocals")
    with pytest.raises(ValueError, match=r"first.output_single_stem is 'Instrumental', so the stem 'Vocals' would never be produced"):
        ChainSeparator(mk("a", output_single_stem="Instrumental"), mk("b"), "Vocals")
    ChainSeparator(mk("a", output_single_stem="vocals"), mk("b"), "Vocals")          # compared without case
    with pytest.raises(ValueError, match=r"the two engines are on different devices \(0 and 1\)"):
        ChainSeparator(mk("a"), mk("b", device=1), "Vocals")
    a = mk("a")
    with pytest.raises(ValueError, match="two plugin instances"):
        ChainSeparator(a, a, "Vocals")
    with pytest.raises(ValueError, match=r"mix-down 'x': 9 terms \(1 .. 8\)"):
        ChainSeparator(mk("a"), mk("b"), "Vocals", mixdowns={"x": [("first", "Vocals", 1.0)] * 9})
    with pytest.raises(ValueError, match=r"stage 'first' or 'then'"):
        ChainSeparator(mk("a"), mk("b"), "Vocals", mixdowns={"x": [("second", "Lead", 1.0)]})
    with pytest.raises(ValueError, match=r"the weight of 'Lead' is not finite"):
        ChainSeparator(mk("a"), mk("b"), "Vocals", mixdowns={"x": [("then", "Lead", float("inf"))]})


def test_unknown_stem_is_refused_at_the_first_file(tmp_path):
    from audio_separator_amd.workflow import ChainSeparator
    path = write_input(tmp_path / "song.wav", 900, 1)
    first, then = make_stage("a", tmp_path / "o", FIRST), make_stage("b", tmp_path / "o", THEN)
    with pytest.raises(ValueError, match=r"'Drums' is not a stem of a: it has \['Vocals', 'Instrumental'\]"):
        ChainSeparator(first, then, "Drums").separate(path)
    assert first.demixes == 0                                                  # known before a sample is touched
    late = make_stage("a", tmp_path / "o", FIRST, late_stems=True)            # a plugin that knows its stems after loading
    with pytest.raises(ValueError, match=r"'Drums' is not a stem a writes for .*song.wav: it wrote \['Vocals', 'Instrumental'\]"):
        ChainSeparator(late, then, "Drums").separate(path)
    assert then.demixes == 0


# ---- the literal flow ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("custom", [None, {"lead": "the lead", "Instrumental": "inst"}])
def test_order_names_and_bytes_are_the_literal_flow(tmp_path, custom, caplog):
    from audio_separator_amd.workflow import ChainSeparator
    path = write_input(tmp_path / "song_(live).wav", 1234, 2)
    want = literal(make_stage("a", tmp_path / "lit", FIRST), make_stage("b", tmp_path / "lit", THEN), path, "Vocals", custom)
    first, then = make_stage("a", tmp_path / "out", FIRST), make_stage("b", tmp_path / "out", THEN)
    chain = ChainSeparator(first, then, "vocals")
    with caplog.at_level(logging.INFO, logger="chain_test"):
        got = chain.separate(path, custom)
    assert got == want and len(got) == 4
    if custom is None:
        assert got[0] == "song_(live)_(Vocals)_a.wav" and got[2] == "song_(live)_(Vocals)_a_(Lead)_b.wav"
    for name in got:
        assert read(tmp_path / "out" / name) == read(tmp_path / "lit" / name), name
    assert chain.last_path_taken == "files" and first.demixes == 1 and then.demixes == 1
    assert sum("chain through the stem's file" in r.getMessage() for r in caplog.records) == 1     # one line saying why
    assert then.audio_file_path == os.path.join(str(tmp_path / "out"), got[0])
    assert first._writer_tap is None and then._writer_tap is None and not then._injected


def test_files_path_when_the_device_decode_declines(tmp_path, monkeypatch, caplog):
    """No refusal up front (as on a machine with a GPU), but the first stage's decoder leaves the file to the host: the device
    writers never meet the stem, and the call is the literal flow."""
    from audio_separator_amd import workflow as W
    monkeypatch.setattr(W.ChainSeparator, "_device_path_refusal", lambda self: None)
    path = write_input(tmp_path / "song.wav", 1000, 3)
    want = literal(make_stage("a", tmp_path / "lit", FIRST), make_stage("b", tmp_path / "lit", THEN), path, "Vocals")
    first, then = make_stage("a", tmp_path / "out", FIRST), make_stage("b", tmp_path / "out", THEN)
    assert first._device_decode(path) is None
    chain = W.ChainSeparator(first, then, "Vocals")
    with caplog.at_level(logging.INFO, logger="chain_test"):
        got = chain.separate(path)
    assert got == want and chain.last_path_taken == "files"
    assert [r.getMessage() for r in caplog.records if "chain through" in r.getMessage()] == [
        f"{path}: chain through the stem's file (the first stage's device writer never saw the Vocals stem (its decoder did not take the file))"]
    for name in got:
        assert read(tmp_path / "out" / name) == read(tmp_path / "lit" / name), name


def test_silent_stem_ends_the_chain(tmp_path):
    from audio_separator_amd.workflow import ChainSeparator
    path = write_input(tmp_path / "song.wav", 800, 4)
    first = make_stage("a", tmp_path / "out", [("Vocals", 0.0), ("Instrumental", 0.6)])
    then = make_stage("b", tmp_path / "out", THEN)
    with pytest.raises(ValueError, match=r"the Vocals stem of .*song.wav is silent: a wrote no file for it"):
        ChainSeparator(first, then, "Vocals").separate(path)
    assert os.path.isfile(tmp_path / "out" / "song_(Instrumental)_a.wav")      # the first stage's other file is there
    assert not os.path.exists(tmp_path / "out" / "song_(Vocals)_a.wav") and then.demixes == 0


# ---- separate_many -----------------------------------------------------------------------------------------------------------------
def test_separate_many_fails_alone_at_either_stage(tmp_path):
    from audio_separator_amd.workflow import ChainSeparator
    paths = [write_input(tmp_path / "one.wav", 1500, 5), str(tmp_path / "missing.wav"), write_input(tmp_path / "short.wav", 300, 6),
             write_input(tmp_path / "four.wav", 1100, 7)]
    loop_first, loop_then = make_stage("a", tmp_path / "loop", FIRST), make_stage("b", tmp_path / "loop", THEN, min_len=500)
    loop = ChainSeparator(loop_first, loop_then, "Vocals", mixdowns={"Both": [("first", "Instrumental", 1.0), ("then", "Backing", 1.0)]})
    want = {}
    for i in (0, 3):
        want[i] = loop.separate(paths[i])
    first, then = make_stage("a", tmp_path / "out", FIRST), make_stage("b", tmp_path / "out", THEN, min_len=500)
    chain = ChainSeparator(first, then, "Vocals", mixdowns={"Both": [("first", "Instrumental", 1.0), ("then", "Backing", 1.0)]})
    got = chain.separate_many(paths)
    assert first.pooled_calls == 1 and then.pooled_calls == 1 and first.demixes == 0 and then.demixes == 0
    assert got[0] == want[0] and got[3] == want[3] and got[0][-1] == "one_(Both)_a+b.wav"
    assert got[1] == [] and 1 in chain.batch_errors                                             # stage one: unreadable
    assert got[2] == ["short_(Vocals)_a.wav", "short_(Instrumental)_a.wav"]                     # stage two: only the first stage's files
    assert isinstance(chain.batch_errors[2], ValueError) and "too short" in str(chain.batch_errors[2])
    assert sorted(chain.batch_errors) == [1, 2] and chain.last_paths_taken == ["files", "failed", "failed", "files"]
    for i in (0, 3):
        for name in got[i]:
            assert read(tmp_path / "out" / name) == read(tmp_path / "loop" / name), name
    # the plugins are left as the loop leaves them: the last good file's sources
    assert np.array_equal(first.primary_source, loop_first.primary_source) and np.array_equal(then.secondary_source, loop_then.secondary_source)


# ---- the door ------------------------------------------------------------------------------------------------------------------------
def test_the_door_is_inert_without_an_injection(tmp_path):
    from audio_separator_amd.common_separator import CommonSeparator
    assert CommonSeparator._injected is None and CommonSeparator._writer_tap is None
    stage = make_stage("a", tmp_path / "out", FIRST)
    path = write_input(tmp_path / "song.wav", 700, 8)
    assert stage._injected_for(path) is None and stage._takes_device_mix() is True
    assert stage._device_mix(path) is None                       # no device file path here: the host decoder's file, as before
    stage.separate(path)
    assert "_injected" not in stage.__dict__ and "_writer_tap" not in stage.__dict__
    out = stage.final_process("x_(Vocals)_a.wav", stage.primary_source, "Vocals")
    assert list(out) == ["Vocals"] and out["Vocals"] is stage.primary_source


def test_an_injected_mix_replaces_the_decode_once(tmp_path):
    stage = make_stage("b", tmp_path / "out", THEN)
    mix = object()
    stage._begin_file("/nowhere/stem.wav")
    stage._inject_mix("/nowhere/stem.wav", mix, {"input_subtype": "PCM_24", "input_bit_depth": 24, "_file_seconds": 2.5, "_file_rate": RATE,
                                                 "_file_frames": 20000}, 0.25)
    assert stage._injected_for("/other.wav") is None
    assert stage._device_mix("/nowhere/stem.wav") is mix
    assert (stage.input_subtype, stage.input_bit_depth, stage._file_seconds, stage._file_rate, stage._file_frames) == ("PCM_24", 24, 2.5, RATE, 20000)
    assert stage._injected_for("/nowhere/stem.wav") is None and stage._device_mix("/nowhere/stem.wav") is None
    stage._inject_mix("/nowhere/zero.wav", mix, {}, 0.0)         # the silent-file refusal of prepare_mix
    with pytest.raises(ValueError, match="Audio file /nowhere/zero.wav is empty or not valid"):
        stage._device_mix("/nowhere/zero.wav")
    stage._inject_mix("/nowhere/zero.wav", mix, {}, 0.0)
    assert stage._device_mix("/nowhere/zero.wav", check_silent=False) is mix


# ---- mix-downs -------------------------------------------------------------------------------------------------------------------------
def test_weight_rule(tmp_path):
    from audio_separator_amd import audio_io
    from audio_separator_amd.workflow import ChainSeparator, mixdown_host, then_weight
    assert then_weight(1.0, 1.0) == np.float32(1.0)
    g = np.float32(0.9) / np.float32(1.37)
    assert then_weight(0.7, g) == np.float32(np.float64(0.7) / np.float64(g)) and then_weight(0.7, g).dtype == np.float32
    # the quotient is taken in float64: the float32 quotient of the rounded operands differs for some weights
    assert any(then_weight(w, g) != np.float32(w) / g for w in np.linspace(0.1, 2.0, 400))
    path = write_input(tmp_path / "song.wav", 1300, 9, scale=0.8)             # Vocals = 1.7 * mix peaks above 0.9: g != 1
    first, then = make_stage("a", tmp_path / "out", FIRST), make_stage("b", tmp_path / "out", THEN)
    chain = ChainSeparator(first, then, "Vocals", mixdowns={"Inst+BV": [("first", "Instrumental", 1.0), ("then", "Backing", 0.75)],
                                                            "Neg": [("then", "Lead", -1.0)]})
    got = chain.separate(path, {"neg": "minus lead"})
    assert got[-2:] == ["song_(Inst+BV)_a+b.wav", "minus lead.wav"]
    handed = first.primary_source
    g = first._normalize_factor(np.abs(handed).max())
    assert chain.last_handoff_gain == g and g < 1.0
    want = mixdown_ref([(first.secondary_source, "rows", 1.0), (then.secondary_source, "rows", then_weight(0.75, g))], 1300, "rows")
    assert np.array_equal(want, mixdown_host([(first.secondary_source, 1.0), (then.secondary_source, then_weight(0.75, g))]))
    then.write_audio("expected.wav", want)
    assert read(tmp_path / "out" / got[-2]) == read(tmp_path / "out" / "expected.wav")
    # at the first stage's scale: Backing / g undoes the factor the second stage heard its input under
    pcm, _ = audio_io.read_wav(str(tmp_path / "out" / got[-2]))
    assert pcm.shape == (2, 1300)


@pytest.mark.parametrize("k", [1, 2, 8])
def test_mixdown_ref_against_exact_sums(k):
    """|err| <= gamma_K * sum |w_k x_k|, gamma_K = K u / (1 - K u), u = 2^-24: the bound of K products and K - 1 additions, each
    rounded once (|x|, |w| <= 4; no term subnormal)."""
    rng = np.random.default_rng(10 + k)
    n_out = 4099
    sources = []
    for i in range(k):
        n = n_out if i % 3 != 2 else n_out - 1000
        mag = np.exp2(rng.uniform(-20, 2, (2, n)))                            # |x| in [2^-20, 4]: products stay far from subnormal
        x = (mag * rng.choice([-1.0, 1.0], (2, n))).astype(np.float32)
        w = np.float32(rng.choice([-1.0, 1.0]) * np.exp2(rng.uniform(-10, 2)))
        sources.append((x if i % 2 == 0 else np.ascontiguousarray(x.T), "planar" if i % 2 == 0 else "rows", w))
    assert all(np.abs(a).max() <= 4 and abs(w) <= 4 for a, _, w in sources)
    got = mixdown_ref(sources, n_out)
    assert got.dtype == np.float32 and got.shape == (2, n_out)
    exact, mass = mixdown_exact(sources, n_out)
    u = 2.0 ** -24
    gamma = k * u / (1 - k * u)
    err = np.abs(got.astype(np.float64) - exact)
    print(f"K={k}: max err / (gamma_K * sum|w x|) = {np.max(err / (gamma * mass)):.3f}")
    assert np.all(err <= gamma * mass)
    assert np.array_equal(mixdown_ref(sources, n_out, "rows"), got.T)


# ---- the C view ------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c_with_the_mix_structs(tmp_path):
    from audio_separator_amd import engine as E
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed for this check"
    # (the array types fail to compile unless the C layout is the one the ctypes mirrors below have)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "asx.h"\n'
           'typedef char src_is_32[(sizeof(asx_mix_src) == 32) ? 1 : -1];\ntypedef char job_is_288[(sizeof(asx_mix_job) == 288) ? 1 : -1];\n'
           'typedef char out_at_264[(offsetof(asx_mix_job, out) == 264) ? 1 : -1];\ntypedef char n_out_at_280[(offsetof(asx_mix_job, n_out) == 280) ? 1 : -1];\n'
           'int main(void) {\n  asx_mix_job j;\n  asx_mix_src s;\n'
           '  int (*f)(asx_engine *, const asx_mix_job *, int32_t, void *) = asx_mixdown_batch_dev;\n'
           '  int (*h)(asx_engine *, const float *const *, const int32_t *, const int64_t *, const float *, int32_t, float *, int32_t, int64_t) = '
           'asx_mixdown;\n  j.k = ASX_MIX_MAX_K;\n  s.layout = ASX_STEM_ROWS;\n'
           '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(s), sizeof(j), offsetof(asx_mix_job, out), offsetof(asx_mix_job, n_out), ASX_ABI_VERSION, '
           'j.k, s.layout);\n  return f == 0 || h == 0;\n}\n')
    c = tmp_path / "mix.c"
    c.write_text(src)
    exe = tmp_path / "mix"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-c", "-o", str(exe) + ".o"],
                   check=True)
    assert C.sizeof(E._MixSrc) == 32 and C.sizeof(E._MixJob) == 288 and E._MixJob.out.offset == 264 and E._MixJob.n_out.offset == 280
    assert [n for n, _ in E._MixSrc._fields_] == ["x", "layout", "n", "w"]
    assert [n for n, _ in E._MixJob._fields_] == ["src", "k", "out", "out_layout", "n_out"]
    assert E.ABI_VERSION == 8 and "asx_mixdown_batch_dev" in E.SYMBOLS and "asx_mixdown" in E.SYMBOLS and E.MIX_MAX_K == 8
    assert hasattr(E.Engine, "mixdown_batch_dev") and hasattr(E.Engine, "mixdown")
    header = open(os.path.join(ROOT, "include", "asx.h")).read()
    assert "#define ASX_MIX_MAX_K 8" in header and "#define ASX_ABI_VERSION 8" in header
