"""``common_config["asx_autocast"]`` on the plugin classes, with the oracle-backed Engine double (tests/fake_engine.py): the knob's values, the
refusals of the plugins whose engines have no single-product kernels, what "follow" does inside and outside ``torch.autocast``, and the engine
option behind it in the library's sources (an option only: no environment name)."""
import os
import re

import numpy as np
import pytest

from tests import fake_engine
from tests import separate_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-audio-separator_amd", "csrc")
REASON = "only the Roformer engine has single-product kernels"


class RecordingEngine(fake_engine.OracleEngine):
    """the double plus ``set_option``: every (key, value) in call order, and the value in force at every demix"""
    options = []
    at_demix = []

    def set_option(self, key, value):
        RecordingEngine.options.append((key, int(value)))
        self._opts = dict(getattr(self, "_opts", {}), **{key: int(value)})

    def rof_demix(self, mix, step):
        RecordingEngine.at_demix.append(getattr(self, "_opts", {}).get("gemm_f16x1"))
        return super().rof_demix(mix, step)

    def rof_demix_batch(self, mixes, step):
        return [self.rof_demix(m, step) for m in mixes]


def _install(monkeypatch, autocast_on=None):
    import torch
    from audio_separator_amd import mdxc
    fake_engine.install(monkeypatch)
    monkeypatch.setattr(mdxc, "Engine", RecordingEngine)
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    RecordingEngine.options, RecordingEngine.at_demix = [], []
    state = {"on": False}
    real = torch.is_autocast_enabled
    # (a GPU-less host cannot enter torch.autocast("cuda"): the query the plugin makes is answered here)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda device_type=None: state["on"] if device_type == "cuda" else real(device_type))
    return state


def _make(tmp_path, family, idx=0, **common_over):
    _, cls, common, arch, wav, _ = SC.cases(family, str(tmp_path))[idx]
    return SC.plugin_class(cls)(common_config=dict(common, **common_over), arch_config=dict(arch)), wav


def test_values():
    from audio_separator_amd.common_separator import CommonSeparator
    assert CommonSeparator.AUTOCAST_MODES == ("off", "fp16", "follow")
    assert CommonSeparator._autocast_mode({}) == "off" and CommonSeparator._autocast_mode({"asx_autocast": None}) == "off"
    for mode in CommonSeparator.AUTOCAST_MODES:
        assert CommonSeparator._autocast_mode({"asx_autocast": mode}) == mode
    for bad in ("on", "bf16", "FP16", True, 1):
        with pytest.raises(ValueError, match="asx_autocast must be one of"):
            CommonSeparator._autocast_mode({"asx_autocast": bad})
    assert CommonSeparator._autocast_refusal is None
    assert CommonSeparator._autocast_active("fp16") and not CommonSeparator._autocast_active("off")


@pytest.mark.parametrize("family", ["mdx", "demucs", "vr"])
def test_fp16_is_refused_where_no_single_product_kernel_exists(tmp_path, monkeypatch, family):
    _install(monkeypatch)
    cls = SC.plugin_class({"mdx": "MDXSeparator", "demucs": "DemucsSeparator", "vr": "VRSeparator"}[family])
    assert cls._autocast_refusal == REASON
    with pytest.raises(ValueError, match=f"asx_autocast='fp16' is not supported by {cls.__name__}: {REASON}"):
        _make(tmp_path, family, asx_autocast="fp16")
    assert fake_engine.OracleEngine.created == 0, "refused at construction, before any engine exists"


def test_fp16_is_refused_for_a_tfc_tdf_model(tmp_path, monkeypatch):
    _install(monkeypatch)
    with pytest.raises(ValueError, match=f"asx_autocast='fp16' is not supported by MDXCSeparator with a TFC-TDF v3 model: {REASON}"):
        _make(tmp_path, "mdxc", asx_autocast="fp16")
    inst, _ = _make(tmp_path, "mdxc", asx_autocast="follow")       # accepted, without effect
    assert inst.asx_autocast == "follow" and RecordingEngine.options == []


def test_follow_is_accepted_and_inert_on_an_mdx_plugin(tmp_path, monkeypatch, caplog):
    """the reference's orchestrator wraps every model's separate() in autocast: "follow" must not make an MDX model raise, or change a byte"""
    import logging
    state = _install(monkeypatch)
    plain, wav = _make(tmp_path, "mdx", output_dir=str(tmp_path / "plain"))
    want = [open(os.path.join(str(tmp_path / "plain"), n), "rb").read() for n in plain.separate(wav, None)]
    with caplog.at_level(logging.INFO):
        inst, _ = _make(tmp_path, "mdx", output_dir=str(tmp_path / "follow"), asx_autocast="follow")
    assert sum("asx_autocast='follow' does nothing on MDXSeparator" in r.getMessage() for r in caplog.records) == 1
    state["on"] = True
    got = [open(os.path.join(str(tmp_path / "follow"), n), "rb").read() for n in inst.separate(wav, None)]   # (the double has no set_option: a call would raise)
    assert got == want and want


def test_follow_sets_the_option_both_ways(tmp_path, monkeypatch):
    """Before every engine call the option is SET -- to 1 inside the context and to 0 outside it, so a "follow" instance is back on the fp32-grade
    kernels after the context; "off" never touches it; "fp16" always sets 1.  ``last_arithmetic`` records it per file."""
    state = _install(monkeypatch)
    inst, wav = _make(tmp_path, "roformer", output_dir=str(tmp_path / "f"), asx_autocast="follow")
    state["on"] = True
    inst.separate(wav, None)
    assert inst.last_arithmetic == "fp16x1" and RecordingEngine.at_demix == [1]
    state["on"] = False
    inst.separate(wav, None)
    assert inst.last_arithmetic == "fp16x3" and RecordingEngine.at_demix == [1, 0], "the option was not set back to 0 outside the context"
    assert RecordingEngine.options and set(RecordingEngine.options) == {("gemm_f16x1", 1), ("gemm_f16x1", 0)}
    assert RecordingEngine.options[-1] == ("gemm_f16x1", 0)
    # separate_many: one arithmetic per call, recorded in every file's state
    state["on"] = True
    RecordingEngine.at_demix = []
    names = inst.separate_many([wav, wav])
    assert all(names) and not inst.batch_errors and set(RecordingEngine.at_demix) == {1} and inst.last_arithmetic == "fp16x1"
    # the host-array entry points take the same setting
    dm = inst._demixer()
    x = (0.3 * np.random.default_rng(1).standard_normal((2, 700))).astype(np.float32)
    state["on"] = False
    dm.demix(x)
    assert dm.last_arithmetic == "fp16x3" and RecordingEngine.options[-1] == ("gemm_f16x1", 0)
    state["on"] = True
    dm.demix_many([x])
    assert dm.last_arithmetic == "fp16x1" and RecordingEngine.options[-1] == ("gemm_f16x1", 1)

    RecordingEngine.options, RecordingEngine.at_demix = [], []
    off, _ = _make(tmp_path, "roformer", output_dir=str(tmp_path / "o"))
    off.separate(wav, None)                                          # inside a live context
    assert off.asx_autocast == "off" and off.last_arithmetic == "fp16x3" and RecordingEngine.options == [] and RecordingEngine.at_demix == [None]

    state["on"] = False
    fp16, _ = _make(tmp_path, "roformer", output_dir=str(tmp_path / "h"), asx_autocast="fp16")
    fp16.separate(wav, None)                                         # outside any context
    assert fp16.last_arithmetic == "fp16x1" and RecordingEngine.at_demix[-1] == 1


def test_the_engine_option_is_an_option_only():
    """asx.hip's option table has "gemm_f16x1"; knobs.h keeps its default in EngineKnobs WITHOUT reading the environment (tests/test_host_knobs.py pins
    the set of environment names); the ABI is still 8 and no symbol was added for it."""
    hip = open(os.path.join(CSRC, "asx.hip")).read()
    assert re.search(r'\{"gemm_f16x1",\s*&asx_engine::gemm_f16x1,\s*&EngineKnobs::gemm_f16x1,\s*opt_onoff\}', hip)
    knobs = open(os.path.join(CSRC, "knobs.h")).read()
    line = [ln for ln in knobs.splitlines() if re.search(r"\bgemm_f16x1\b", ln)]
    assert len(line) == 1 and re.match(r"\s*int gemm_f16x1 = 0;", line[0]), line
    assert "knob::" not in line[0] and "getenv" not in line[0] and "ASX_GEMM_F16X1" not in knobs + hip
    header = open(os.path.join(ROOT, "include", "asx.h")).read()
    assert re.search(r"#define ASX_ABI_VERSION\s+8\b", header)
    assert '"gemm_f16x1"' in header and "f16x1" not in "".join(re.findall(r"^int asx_\w+\(", header, re.M))
    for name in ("tdf3s_launches", "attn6s_launches"):
        assert f'"{name}"' in hip and f'"{name}"' in header
    from audio_separator_amd.engine import ATTN_VARIANTS
    names = re.search(r"k_attn_variant_names\[AV_COUNT\] = \{(.*?)\};", open(os.path.join(CSRC, "engine_attn.h")).read(), re.S).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == ATTN_VARIANTS and ATTN_VARIANTS[-2:] == ("attn6s", "attn6s_qw2")
