"""CPU side of the multi-model ensemble (audio_separator_amd/ensemble.py): the stem-name rule, output naming, weight
fallbacks, constructor refusals and the choice between the device path and the file path -- the last with the plugin classes
driven by the Engine double of tests/fake_engine.py, which has no device decoder, so every input takes the file path.

The hand tables are read off the reference's ``Separator._separate_ensemble`` (separator.py:1288-1368) and
``Ensembler.ensemble`` (ensembler.py:32-44)."""
import logging
import os
import sys
import types

import numpy as np
import pytest

from oracle import ensemble_oracle as EO
from tests import fake_engine, separate_cases as SC

from audio_separator_amd import EnsembleSeparator, Ensembler, Engine
from audio_separator_amd import ensemble as ENS
from audio_separator_amd import plugin


# ---- stem names --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw, want", [
    (["Vocals", "Instrumental"], ["Vocals", "Instrumental"]),
    (["vocals", "other"], ["Vocals", "Instrumental"]),                      # "other" beside a vocal stem in a 2-stem model
    (["drums", "other"], ["Drums", "Other"]),                               # no vocal sibling: stays Other
    (["Bass", "Drums", "Other", "Vocals"], ["Bass", "Drums", "Other", "Vocals"]),   # 4 stems: Other stays Other
    (["vocals_lead", "Vocals"], ["Vocals_Lead", "Vocals"]),                 # lead / backing stay apart from Vocals
    (["Backing Vocals", "Lead Vocals"], ["Backing Vocals", "Lead Vocals"]),
    (["no_vocals", "Vocals"], ["Vocals", "Vocals"]),                        # contains "vocal": the first rule wins, as in the reference
    (["inst", "karaoke"], ["Instrumental", "Instrumental"]),
    (["No Drums", "weird stem"], ["No Drums", "Weird Stem"]),               # unknown -> .title()
    (["male vocal"], ["Vocals"]),
])
def test_canonical_stem_names(raw, want):
    assert ENS.canonical_stem_names(raw) == want


def test_raw_stem_name_takes_the_first_parenthesis():
    assert ENS.raw_stem_name("song_(Vocals)_model.wav") == "Vocals"
    assert ENS.raw_stem_name("/tmp/x/song_(No Drums)_m.flac") == "No Drums"
    # an input that itself carries "_(...)": every stem of it reads as that label (the reference's regex, kept)
    assert ENS.raw_stem_name("song_(live)_(Vocals)_model.wav") == "live"
    assert ENS.raw_stem_name("song_(live)_(Instrumental)_model.wav") == "live"
    assert ENS.raw_stem_name("plain.wav") == "Unknown"
    assert ENS.canonical_stem_names(["live", "live"]) == ["Live", "Live"]


# ---- output names -------------------------------------------------------------------------------------------------
def test_output_names():
    files = ["model_bs_roformer_ep_317_sdr_12.9755.ckpt", "UVR-MDX-NET-Inst_HQ_3.onnx", "bs_roformer_x.ckpt", "htdemucs_ft.yaml",
             "mel_band_roformer_karaoke_aufr33_viperx.ckpt"]
    assert ENS.model_slugs(files) == "ep_317_sdr_1_Inst_HQ_3_x_htdemucs_ft_karaoke_aufr"
    assert ENS.ensemble_output_name("song", "Vocals", None, None, files[:2]) == "song_(Vocals)_custom_ensemble_ep_317_sdr_1_Inst_HQ_3"
    assert ENS.ensemble_output_name("song", "Vocals", None, "vocal_balanced", files) == "song_(Vocals)_preset_vocal_balanced"
    assert ENS.ensemble_output_name("song", "Vocals", {"Vocals": "lead"}, "p", files) == "lead"
    # the reference looks the group name up as it is (no lower-casing): another key does not apply
    assert ENS.ensemble_output_name("song", "Vocals", {"vocals": "lead"}, "p", files) == "song_(Vocals)_preset_p"
    # only the first matching prefix is removed
    assert ENS.model_slugs(["UVR_MDXNET_UVR-MDX-NET-a.onnx"]) == "UVR-MDX-NET-"


# ---- weights ------------------------------------------------------------------------------------------------------
def test_weight_fallbacks():
    ones = [1.0, 1.0, 1.0]
    assert list(ENS.effective_weights(None, 3)) == ones
    assert list(ENS.effective_weights([1.0, 2.0, 0.5], 3)) == [1.0, 2.0, 0.5]
    assert list(ENS.effective_weights([1.0, 2.0], 3)) == ones                    # length mismatch
    assert list(ENS.effective_weights([1.0, float("nan"), 1.0], 3)) == ones      # non-finite
    assert list(ENS.effective_weights([1.0, float("inf"), 1.0], 3)) == ones
    assert list(ENS.effective_weights([1.0, -1.0, 0.0], 3)) == ones              # zero sum
    # the engine-side helper of ensemble_dev agrees (None = equal weights)
    assert Engine.ensemble_weights(None, 3) is None
    assert Engine.ensemble_weights([1.0, 2.0, 0.5], 3) == [1.0, 2.0, 0.5]
    for bad in ([1.0, 2.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], [1.0, -1.0, 0.0]):
        assert Engine.ensemble_weights(bad, 3) is None


def test_ensembler_host_branches():
    log = logging.getLogger("t")
    e = Ensembler(log, "avg_wave", [1.0, 3.0])
    assert e.ensemble([]) is None
    w = np.ones((2, 5), np.float32)
    assert e.ensemble([w]) is w
    with pytest.raises(ValueError, match="same number of channels"):
        e.ensemble([np.ones((2, 5), np.float32), np.ones((1, 5), np.float32)])
    # mono waves: the numpy restatement, ragged lengths zero padded
    a, b = np.full((1, 4), 1.0, np.float32), np.full((1, 6), 2.0, np.float32)
    got = e.ensemble([a, b])
    assert got.shape == (1, 6) and np.allclose(got[0], [1.75] * 4 + [1.5] * 2)
    rng = np.random.default_rng(0)
    ws = [rng.standard_normal((1, 50)).astype(np.float32) for _ in range(3)]
    for alg in ("median_wave", "min_wave", "max_wave"):
        assert np.array_equal(Ensembler(log, alg).ensemble(ws), EO.ensemble(ws, alg))
    with pytest.raises(ValueError):
        Ensembler(log, "nope").ensemble(ws)


# ---- registration ---------------------------------------------------------------------------------------------------
def test_install_registers_the_ensembler_only_on_request(monkeypatch):
    name = "audio_separator.separator.ensembler"
    for k in [k for k in sys.modules if k.startswith("audio_separator.")]:
        monkeypatch.delitem(sys.modules, k)
    try:
        plugin.install()
        assert name not in sys.modules
        orch = types.ModuleType("audio_separator.separator.separator")
        orch.Ensembler = previous = object()
        monkeypatch.setitem(sys.modules, "audio_separator.separator.separator", orch)
        assert name in plugin.install(ensembler=True)
        assert sys.modules[name].Ensembler is Ensembler and orch.Ensembler is Ensembler
        plugin.uninstall()
        assert name not in sys.modules and orch.Ensembler is previous
        plugin.install()
        assert name not in sys.modules
    finally:
        plugin.uninstall()


# ---- constructor -----------------------------------------------------------------------------------------------------
def _stub(**over):
    m = types.SimpleNamespace(sample_rate=44100, normalization_threshold=0.9, amplification_threshold=0.0, use_soundfile=False,
                              output_dir="out", output_format="WAV", model_path="/m/UVR-MDX-NET-a_long_model_name.onnx",
                              model_name="a", logger=logging.getLogger("t"), engine=None)
    m.stems_dev = lambda path: None
    for k, v in over.items():
        setattr(m, k, v)
    return m


def test_constructor_refusals():
    with pytest.raises(ValueError, match="at least one"):
        EnsembleSeparator([])
    with pytest.raises(ValueError, match="Unknown ensemble algorithm"):
        EnsembleSeparator([_stub()], algorithm="nope")
    for key, other in (("sample_rate", 8000), ("normalization_threshold", 0.8), ("amplification_threshold", 0.1)):
        with pytest.raises(ValueError, match=key):
            EnsembleSeparator([_stub(), _stub(**{key: other})])
    with pytest.raises(ValueError, match="intermediate"):
        EnsembleSeparator([_stub()], intermediate="int8")
    with pytest.raises(ValueError, match="device path"):
        EnsembleSeparator([_stub()], intermediate="float32", via_files=True)
    with pytest.raises(ValueError, match="model file names"):
        EnsembleSeparator([_stub(), _stub()], model_filenames=["a.onnx"])
    ens = EnsembleSeparator([_stub(), _stub(model_path=None, model_name="htd")])
    assert ens.model_filenames == ["UVR-MDX-NET-a_long_model_name.onnx", "htd"]
    assert ENS.model_slugs(ens.model_filenames) == "a_long_model_htd"


def test_device_path_refusals():
    assert EnsembleSeparator([_stub(), _stub()])._device_path_refusal() is None
    assert "via_files" in EnsembleSeparator([_stub()], via_files=True)._device_path_refusal()
    assert "soundfile" in EnsembleSeparator([_stub(), _stub(use_soundfile=True)])._device_path_refusal()
    assert "output_format" in EnsembleSeparator([_stub(), _stub(output_format="MP3")])._device_path_refusal()
    assert EnsembleSeparator([_stub(output_format="FLAC"), _stub(output_format="flac")])._device_path_refusal() is None


# ---- path selection with real plugin classes on the Engine double -------------------------------------------------------
class _EnsembleOracleEngine(fake_engine.OracleEngine):
    def ensemble(self, waveforms, algorithm="avg_wave", weights=None):
        ws = [np.asarray(w, np.float32) for w in waveforms]
        if len(ws) == 1:
            return ws[0]
        n = max(w.shape[1] for w in ws)
        w = ENS.effective_weights(weights, len(ws))
        return np.asarray(EO.ensemble([np.pad(x, ((0, 0), (0, n - x.shape[1]))) for x in ws], algorithm, list(w)), np.float32)


def _members(tmp, monkeypatch, **mdx_over):
    fake_engine.install(monkeypatch)
    from audio_separator_amd import demucs, mdx, mdxc, vr
    for mod in (mdx, mdxc, demucs, vr):
        monkeypatch.setattr(mod, "Engine", _EnsembleOracleEngine)
    mdx_case, mdxc_case = SC.cases("mdx", tmp)[0], SC.cases("mdxc", tmp)[1]
    out = []
    for (_, cls, common, arch, _, _), over in ((mdx_case, mdx_over), (mdxc_case, {})):
        out.append(SC.plugin_class(cls)(common_config=dict(common, **over), arch_config=arch))
    return out, mdx_case[4]


def test_file_path_is_taken_without_a_device_decoder(tmp_path, monkeypatch, caplog):
    """The double has no asx_pcm_decode_dev, so ``stems_dev`` returns None like ``_device_mix`` does and the input goes through
    intermediate files; the combine is the weighted average of the files read back, written by the last member."""
    from audio_separator_amd import audio_io
    members, wav = _members(str(tmp_path), monkeypatch)
    assert all(m.stems_dev(wav) is None for m in members)
    ens = EnsembleSeparator(members, "avg_wave", [1.0, 3.0], model_filenames=["UVR-MDX-NET-net_small_long_name.onnx", "mdxc_v3one.ckpt"])
    ens.output_dir = str(tmp_path / "final")
    written = []
    for m in members:
        real = m.write_audio
        monkeypatch.setattr(m, "write_audio", lambda p, s, real=real, m=m: (written.append((m, p, m.output_dir)), real(p, s))[1])
    with caplog.at_level(logging.INFO):
        files = ens.separate(wav)
    assert ens.last_path_taken == "files" and "needs the host decoder" in caplog.text
    stem = "custom_ensemble_net_small_lo_mdxc_v3one"
    assert files == [os.path.join(ens.output_dir, f"mdx_in_({s})_{stem}.wav") for s in ("Instrumental", "Vocals")]
    # two intermediates per member into the temporary directory (gone now), two results by the last member into output_dir
    assert [w[0] for w in written].count(members[0]) == 2 and [w[0] for w in written].count(members[1]) == 4
    finals = [w for w in written if w[2] == ens.output_dir]
    assert [w[0] for w in finals] == [members[1]] * 2 and all(not os.path.exists(w[2]) for w in written if w[2] != ens.output_dir)
    assert members[0].output_dir == os.path.join(str(tmp_path), "out")          # a member's own output_dir is put back
    for f in files:
        x, sr = audio_io.read_wav(f)
        assert sr == 44100 and x.shape == (2, 3000) and np.abs(x).max() > 1e-4
    # the same call again gives the same bytes; a list of inputs gives the outputs of all of them
    first = [open(f, "rb").read() for f in files]
    assert ens.separate([wav, wav]) == files + files
    assert [open(f, "rb").read() for f in files] == first


def test_single_stem_member_and_custom_names_on_the_file_path(tmp_path, monkeypatch):
    members, wav = _members(str(tmp_path), monkeypatch, output_single_stem="instrumental")
    ens = EnsembleSeparator(members, "max_wave", preset="karaoke", via_files=True)
    ens.output_dir = str(tmp_path / "final")
    files = ens.separate(wav, {"Vocals": "only_vocals"})
    assert files == [os.path.join(ens.output_dir, "mdx_in_(Instrumental)_preset_karaoke.wav"), os.path.join(ens.output_dir, "only_vocals.wav")]
    assert all(os.path.isfile(f) for f in files)
