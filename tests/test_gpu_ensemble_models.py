"""Multi-model ensembles on the MI355X (audio_separator_amd/ensemble.py, asx_ensemble_slot_dev).

1. the member -> Ensembler edge (asx_ensemble_slot_dev) against its definition -- the int16 the writer kernels produce for the
   same stem, read back as ``int16 / 32768``, transposed and zero padded -- bit for bit;
2. the device path of ``EnsembleSeparator`` against its file path (``via_files=True``: resident members, 16-bit intermediate
   files, ``Engine.ensemble`` on the host arrays -- all pieces pinned to reference goldens elsewhere), byte for byte, for all
   eleven algorithms;
3. members with unequal stem lengths and groups with a single contributor (Demucs + VR at 8 kHz);
4. options (single stem, output names, the soundfile fallback, repeatability);
5. the drop-in ``Ensembler`` against the reference's golden vectors."""
import filecmp
import logging
import os
import random
import sys
import tempfile

import numpy as np
import pytest

from oracle import ensemble_oracle as EO
from tests import separate_cases as SC

pytestmark = pytest.mark.gpu

ALGORITHMS = ("avg_wave", "median_wave", "min_wave", "max_wave", "avg_fft", "median_fft", "min_fft", "max_fft", "uvr_max_spec",
              "uvr_min_spec", "ensemble_wav")


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    return A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))


# ---- 1. the slot edge ------------------------------------------------------------------------------------------------
MAX_PEAK = 0.9
# (name, amplitude of the loudest sample, min_peak): above max_peak / below a set min_peak / between the two / all zeros
REGIMES = (("above", 1.7, None), ("below", 0.2, 0.5), ("between", 0.7, 0.5), ("zeros", 0.0, 0.0))


def _stem(n, amplitude, seed):
    rng = np.random.default_rng(seed)
    x = (amplitude * rng.uniform(-1.0, 1.0, (2, n))).astype(np.float32)
    x[n % 2, n // 2] = -amplitude             # the peak is exactly the regime's amplitude, whatever n
    return x


@pytest.mark.parametrize("layout", ["planar", "rows"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_slot_edge_is_the_pcm16_round_trip(eng, n, layout):
    import torch
    dev = torch.device("cuda", 0)
    for r, (regime, amplitude, min_peak) in enumerate(REGIMES):
        x = _stem(n, amplitude, 100 * n + r)
        stem = torch.from_numpy(np.ascontiguousarray(x if layout == "planar" else x.T)).to(dev)
        pcm = torch.empty((n, 2), dtype=torch.int16, device=dev)
        quantise = eng.pcm16_planar_dev if layout == "planar" else eng.pcm16_rows_dev
        peak_ref = quantise(stem.data_ptr(), n, MAX_PEAK, min_peak, pcm.data_ptr())
        torch.cuda.synchronize()
        back = (pcm.cpu().numpy().astype(np.float32) / 32768).T             # librosa.load of the 16-bit file, [2, n]
        for n_max in (n, n + 300):
            want = np.zeros((2, n_max), np.float32)
            want[:, :n] = back
            stack = torch.full((3, 2, n_max), float("nan"), dtype=torch.float32, device=dev)
            peak = eng.ensemble_slot_dev(stem.data_ptr(), n, layout, MAX_PEAK, min_peak, stack.data_ptr(), 1, n_max)
            got = stack.cpu().numpy()
            assert np.array_equal(got[1], want), (regime, n_max)
            assert np.isnan(got[0]).all() and np.isnan(got[2]).all(), (regime, n_max)      # the neighbours are not touched
            assert peak == peak_ref, (regime, peak, peak_ref)
            # float32: a bitwise copy (transposed for rows) plus zeros, no normalisation
            stack.fill_(float("nan"))
            peak32 = eng.ensemble_slot_dev(stem.data_ptr(), n, layout, MAX_PEAK, min_peak, stack.data_ptr(), 2, n_max, mode="float32")
            got = stack.cpu().numpy()
            assert np.array_equal(got[2, :, :n].view(np.uint32), x.view(np.uint32)) and not got[2, :, n:].any(), (regime, n_max)
            assert np.isnan(got[:2]).all() and peak32 == np.float32(np.abs(x).max())
        if regime == "above":
            assert peak_ref == pytest.approx(MAX_PEAK, rel=1e-6) and np.abs(back).max() <= MAX_PEAK
        elif regime == "below":
            assert peak_ref == pytest.approx(0.5, rel=1e-6)
        elif regime == "zeros":
            assert peak_ref == 0.0 and not back.any()


def test_slot_edge_refuses_bad_arguments(eng):
    import torch
    import audio_separator_amd as A
    dev = torch.device("cuda", 0)
    stem = torch.ones((2, 64), dtype=torch.float32, device=dev)
    stack = torch.full((2, 2, 64), float("nan"), dtype=torch.float32, device=dev)
    for args, kw in (((stem.data_ptr(), 65, "planar", 0.9, 0.0, stack.data_ptr(), 0, 64), {}),          # n > n_max
                     ((0, 64, "planar", 0.9, 0.0, stack.data_ptr(), 0, 64), {}),                        # null stem
                     ((stem.data_ptr(), 64, "planar", 0.9, 0.0, 0, 0, 64), {}),                         # null stack
                     ((stem.data_ptr(), 64, "rows", 0.9, 0.0, stack.data_ptr(), -1, 64), {}),           # k < 0
                     ((stem.data_ptr(), -1, "rows", 0.9, 0.0, stack.data_ptr(), 0, 64), {})):           # n < 0
        with pytest.raises(A.AsxError, match="asx_ensemble_slot_dev"):
            eng.ensemble_slot_dev(*args, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(stack).all()
    # n == 0: the slot is all padding
    assert eng.ensemble_slot_dev(0, 0, "planar", 0.9, 0.0, stack.data_ptr(), 1, 64) == 0.0
    got = stack.cpu().numpy()
    assert not got[1].any() and np.isnan(got[0]).all()


# ---- members -----------------------------------------------------------------------------------------------------------
def _member(case, **over):
    _, cls, common, arch, _, _ = case
    return SC.plugin_class(cls)(common_config=dict(common, **over), arch_config=arch)


@pytest.fixture(scope="module")
def members_44k(tmp_path_factory):
    """MDX (ConvTDFNet .onnx), MDXC (TFC-TDF v3, single target + residual) and BS-Roformer at 44.1 kHz."""
    tmp = str(tmp_path_factory.mktemp("ens44"))
    cases = [SC.cases("mdx", tmp)[0], SC.cases("mdxc", tmp)[1], SC.cases("roformer", tmp)[0]]
    return [_member(c) for c in cases], os.path.join(SC.AUDIO, "mdx_in.wav")


@pytest.fixture(scope="module")
def members_8k(tmp_path_factory):
    """HTDemucs (4 stems, N samples) and a VR net (2 stems, shorter) at 8 kHz."""
    tmp = str(tmp_path_factory.mktemp("ens8"))
    cases = [SC.cases("demucs", tmp)[0], SC.cases("vr", tmp)[0]]
    return [_member(c) for c in cases], os.path.join(SC.AUDIO, "vr_in.wav")


def _count_writes(members, monkeypatch):
    counts = [0] * len(members)
    for i, m in enumerate(members):
        real = m.write_audio

        def write_audio(path, source, real=real, i=i):
            counts[i] += 1
            real(path, source)
        monkeypatch.setattr(m, "write_audio", write_audio)
    return counts


def _both_paths(members, wav, tmp_path, monkeypatch, algorithm, weights=None, custom=None, **kw):
    """Run the file path, then the device path (no temporary directory allowed, members write final outputs only); returns the
    relative names after asserting that both wrote the same names and the same bytes."""
    import audio_separator_amd as A
    by_files = A.EnsembleSeparator(members, algorithm, weights, via_files=True, **kw)
    by_files.output_dir = str(tmp_path / "files")
    want = by_files.separate(wav, custom)
    assert by_files.last_path_taken == "files" and want

    on_device = A.EnsembleSeparator(members, algorithm, weights, **kw)
    on_device.output_dir = str(tmp_path / "device")
    with monkeypatch.context() as mp:
        def no_temp_dir(*a, **k):
            raise AssertionError("the device path must not create a temporary directory")
        mp.setattr(tempfile, "mkdtemp", no_temp_dir)
        counts = _count_writes(members, mp)
        got = on_device.separate(wav, custom)
    assert on_device.last_path_taken == "device"
    assert counts == [0] * (len(members) - 1) + [len(got)], counts        # only final outputs, by the last member
    rel_want = [os.path.relpath(f, by_files.output_dir) for f in want]
    rel_got = [os.path.relpath(f, on_device.output_dir) for f in got]
    assert rel_got == rel_want
    for a, b in zip(got, want):
        assert os.path.isfile(a) and os.path.isfile(b), (a, b)
        assert filecmp.cmp(a, b, shallow=False), (algorithm, os.path.basename(a))
    return rel_got, got


# ---- 2. device path == file path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_device_path_equals_file_path(members_44k, tmp_path, monkeypatch, algorithm):
    from audio_separator_amd import audio_io
    members, wav = members_44k
    weights = [1.0, 2.0, 0.5] if algorithm.startswith("avg_") else None
    names, files = _both_paths(members, wav, tmp_path, monkeypatch, algorithm, weights)
    slugs = "net_small_mdxc_v3one_small"          # net_small.onnx, mdxc_v3one.ckpt, model_bs_roformer_small.ckpt (prefix dropped)
    assert names == [f"mdx_in_({s})_custom_ensemble_{slugs}.wav" for s in ("Instrumental", "Vocals")]
    n = 3000 if not algorithm.startswith("uvr_") else 1024 * (3000 // 1024)
    for f in files:
        x, sr = audio_io.read_wav(f)
        assert sr == 44100 and x.shape == (2, n) and np.abs(x).max() > 1e-4


# ---- 3. unequal lengths, lone groups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["avg_wave", "uvr_max_spec"])
def test_unequal_lengths_and_lone_groups(members_8k, tmp_path, monkeypatch, algorithm):
    from audio_separator_amd import audio_io
    members, wav = members_8k
    monkeypatch.setattr(random, "randint", lambda a, b: a + (b - a) // 3)      # the Demucs shift draws, the same on both paths
    names, files = _both_paths(members, wav, tmp_path, monkeypatch, algorithm)
    # Demucs writes Bass, Drums, Other, Vocals; VR its primary (Instrumental) first, then Vocals: Vocals has two contributors
    slugs = "htd_single_vr_small_311"
    assert names == [f"vr_in_({s})_custom_ensemble_{slugs}.wav" for s in ("Bass", "Drums", "Other", "Vocals", "Instrumental")]
    n_demucs = audio_io.wav_info(wav)["frames"]
    lengths = {os.path.basename(f).split("_(")[1].split(")")[0]: audio_io.wav_info(f)["frames"] for f in files}
    n_vr = lengths["Instrumental"]
    assert n_vr != n_demucs and lengths["Bass"] == lengths["Drums"] == lengths["Other"] == n_demucs   # lone groups: untouched lengths
    longest = max(n_vr, n_demucs)
    assert lengths["Vocals"] == (longest if algorithm == "avg_wave" else 1024 * (longest // 1024))


# ---- 4. options --------------------------------------------------------------------------------------------------------
def test_options(tmp_path, monkeypatch, caplog):
    import audio_separator_amd as A
    tmp = str(tmp_path)
    wav = os.path.join(SC.AUDIO, "mdx_in.wav")
    mdx_case, mdxc_case = SC.cases("mdx", tmp)[0], SC.cases("mdxc", tmp)[1]
    single, full = _member(mdx_case, output_single_stem="instrumental"), _member(mdxc_case)
    # one member gives only its Instrumental: that group has two contributors, Vocals one; custom name for one, preset for the other
    names, _ = _both_paths([single, full], wav, tmp_path / "a", monkeypatch, "max_fft", custom={"Vocals": "just_vocals"}, preset="duo")
    assert names == ["mdx_in_(Instrumental)_preset_duo.wav", "just_vocals.wav"]
    # slug naming with a prefixed, long model name; float32 intermediates also run on the device
    filenames = ["UVR-MDX-NET-a_very_long_model_name.onnx", "mdxc_v3one.ckpt"]
    names, first = _both_paths([single, full], wav, tmp_path / "b", monkeypatch, "avg_wave", [3.0, 1.0], model_filenames=filenames)
    assert names == [f"mdx_in_({s})_custom_ensemble_a_very_long__mdxc_v3one.wav" for s in ("Instrumental", "Vocals")]
    # two calls give identical bytes
    kept = [open(f, "rb").read() for f in first]
    again = A.EnsembleSeparator([single, full], "avg_wave", [3.0, 1.0], model_filenames=filenames)
    again.output_dir = str(tmp_path / "b" / "device")
    assert again.separate([wav]) == first and again.last_path_taken == "device"
    assert [open(f, "rb").read() for f in first] == kept
    exact = A.EnsembleSeparator([single, full], "avg_wave", intermediate="float32")
    exact.output_dir = str(tmp_path / "c")
    out = exact.separate(wav)
    assert exact.last_path_taken == "device" and len(out) == 2 and all(os.path.isfile(f) for f in out)
    # a member that writes with soundfile sends the input through the file path
    sf_member = _member(mdx_case, use_soundfile=True)
    ens = A.EnsembleSeparator([sf_member, full], "avg_wave")
    ens.output_dir = str(tmp_path / "d")
    with caplog.at_level(logging.INFO):
        out = ens.separate(wav)
    assert ens.last_path_taken == "files" and "soundfile" in caplog.text and len(out) == 2 and all(os.path.isfile(f) for f in out)


# ---- 5. the drop-in Ensembler ------------------------------------------------------------------------------------------------
def _rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("alg", EO.ALGORITHMS)
def test_ensembler_dropin_golden(golden_dir, alg):
    """The tolerances of tests/test_gpu_ensemble.py for ``Engine.ensemble``."""
    import audio_separator_amd as A
    g = np.load(os.path.join(golden_dir, "ensemble_small.npz"))
    w = [g["waves"][k] for k in range(4)]
    log = logging.getLogger("ensembler")
    tol = 0.0 if alg in ("median_wave", "min_wave", "max_wave", "ensemble_wav") else 5e-6
    assert _rel(A.Ensembler(log, alg).ensemble(w), g[f"{alg}_k4"]) <= tol
    assert _rel(A.Ensembler(log, algorithm=alg, weights=None).ensemble(w[:3]), g[f"{alg}_k3"]) <= tol
    if alg in ("avg_wave", "avg_fft"):
        assert _rel(A.Ensembler(log, alg, [1.0, 2.0, 0.5, 0.25]).ensemble(w), g[f"{alg}_w"]) < 5e-6
        assert _rel(A.Ensembler(log, alg, [1.0, 2.0]).ensemble(w), g[f"{alg}_k4"]) <= tol          # length mismatch: equal weights
    assert A.Ensembler(log, alg).ensemble([]) is None and A.Ensembler(log, alg).ensemble([w[0]]) is w[0]


def test_ensembler_registration():
    import audio_separator_amd as A
    name = "audio_separator.separator.ensembler"
    saved = {k: v for k, v in sys.modules.items() if k.startswith("audio_separator.")}
    try:
        A.uninstall()
        A.install()
        assert name not in sys.modules
        assert name in A.install(ensembler=True) and sys.modules[name].Ensembler is A.Ensembler
        A.uninstall()
        assert name not in sys.modules
    finally:
        A.uninstall()
        sys.modules.update(saved)
