"""use_soundfile=True with the stems still in HBM (CommonSeparator._write_soundfile_device), soundfile patched absent: the samples are converted
to the file's own format on the device (asx_pcm_encode_dev) and only the file's bytes -- or, for a .flac name, the frames of
asx_flac_encode_pcm_dev -- come back.  The yardstick is the code the class had before, which ASX_FILE_FASTPATH=0 still runs: host stems,
Engine.normalize, audio_io.write_wav.  Both compute the same IEEE operations, so the files are compared byte for byte.
`mdx` stems are rows [N, 2] in HBM, `demucs` stems planar [2, N]; of the demucs cases the one without random shifts, whose runs repeat."""
import logging
import os

import numpy as np
import pytest

from tests import flac_ref as F
from tests import separate_cases as SC

pytestmark = pytest.mark.gpu

SUBTYPES = ("PCM_16", "PCM_24", "PCM_32", "FLOAT")
FAMILIES = {"mdx": 0, "demucs": 2}          # the case of tests/separate_cases.py


@pytest.fixture(scope="module")
def no_soundfile():
    from audio_separator_amd import audio_io
    real = audio_io._optional
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(audio_io, "_optional", lambda name: None if name == "soundfile" else real(name))
        mp.delenv("ASX_OUTPUT_ENCODER", raising=False)
        yield mp


class Runs:
    """one plugin instance of a family; every (mode, subtype) separated once"""

    def __init__(self, family, tmp, mp):
        from audio_separator_amd import audio_io
        self.tmp = tmp
        _, cls, common, arch, wav, _ = SC.cases(family, tmp)[FAMILIES[family]]
        x, self.rate = audio_io.read_wav(wav)
        self.inputs = {}
        for st in SUBTYPES:
            self.inputs[st] = os.path.join(tmp, f"in_{st}.wav")
            audio_io.write_wav(self.inputs[st], np.ascontiguousarray(x.T), self.rate, st)
        self.inst = SC.plugin_class(cls)(common_config=dict(common, use_soundfile=True), arch_config=arch)
        self.mp = mp
        self.done = {}
        for mode, env in (("fast", {}), ("host", {"ASX_FILE_FASTPATH": "0"}), ("sync", {"ASX_ASYNC_WRITES": "0"})):
            for st in SUBTYPES:
                self.done[mode, st] = self.separate(self.inputs[st], mode, env)
        self.inst.output_dir = os.path.join(tmp, "many")
        self.inst.last_write_path = None
        lists = self.inst.separate_many([self.inputs[st] for st in SUBTYPES])
        self.many = {st: self._blobs(names) for st, names in zip(SUBTYPES, lists)}
        self._reset()

    def _blobs(self, names):
        out = {}
        for n in names:
            path = os.path.join(self.inst.output_dir, n)
            if os.path.exists(path):                   # (a refused stem leaves its name and no file)
                with open(path, "rb") as f:
                    out[n] = f.read()
        return out

    def _reset(self):
        self.left = dict(self.inst._dev_stems)
        self.inst.clear_gpu_cache()
        self.inst.clear_file_specific_paths()

    def separate(self, path, mode, env=None, fmt="WAV"):
        inst = self.inst
        inst.output_dir = os.path.join(self.tmp, mode + "_" + fmt)
        inst.output_format = fmt
        inst.last_write_path = None
        with self.mp.context() as m:
            for k in ("ASX_FILE_FASTPATH", "ASX_ASYNC_WRITES"):
                m.delenv(k, raising=False)
            for k, v in (env or {}).items():
                m.setenv(k, v)
            names = inst.separate(path, None)
        got = {"names": names, "blobs": self._blobs(names), "timings": dict(inst.file_timings), "how": inst.last_write_path,
               "paths": [os.path.join(inst.output_dir, n) for n in names]}
        self._reset()
        got["left"] = self.left
        return got


@pytest.fixture(scope="module", params=list(FAMILIES))
def runs(request, tmp_path_factory, no_soundfile):
    return Runs(request.param, str(tmp_path_factory.mktemp("sfw_" + request.param)), no_soundfile)


@pytest.mark.parametrize("subtype", SUBTYPES)
def test_wav_stems_equal_the_host_path(runs, subtype):
    from audio_separator_amd import audio_io
    fast, host = runs.done["fast", subtype], runs.done["host", subtype]
    assert len(fast["names"]) >= 2 and fast["names"] == host["names"] and sorted(fast["blobs"]) == sorted(fast["names"])
    for n in fast["names"]:
        assert fast["blobs"][n] == host["blobs"][n], (subtype, n)
        assert audio_io.info(os.path.join(runs.tmp, "fast_WAV", n))["subtype"] == subtype
    assert fast["how"] == "wav_device_resident" and fast["timings"].get("pcm_encode_d2h", 0.0) > 0.0
    assert host["how"] is None and "pcm_encode_d2h" not in host["timings"]
    assert fast["left"] == {}


@pytest.mark.parametrize("subtype", SUBTYPES)
def test_synchronous_writes_and_separate_many_give_the_same_bytes(runs, subtype):
    fast, sync = runs.done["fast", subtype], runs.done["sync", subtype]
    assert sync["how"] == "wav_device_resident" and sync["blobs"] == fast["blobs"]
    assert runs.many[subtype] == fast["blobs"]


@pytest.mark.parametrize("subtype,bits", [("PCM_24", 24), ("PCM_16", 16)])
def test_flac_stems_keep_the_real_bits(runs, subtype, bits):
    from audio_separator_amd import audio_io
    got = runs.separate(runs.inputs[subtype], "fast", fmt="FLAC")
    wavs = runs.done["fast", subtype]
    assert got["how"] == "flac_device_resident" and got["timings"].get("flac_encode", 0.0) > 0.0 and got["left"] == {}
    assert len(got["paths"]) == len(wavs["paths"]) >= 2
    wide = False
    for fp, wp in zip(got["paths"], wavs["paths"]):
        assert fp.endswith(".flac") and wp.endswith(".wav")
        with open(fp, "rb") as f:
            data = f.read()
        info, pcm, frames = F.decode(data)                                   # raises on any CRC mismatch
        x, _ = audio_io.read_wav(wp)
        want = np.rint(x.T.astype(np.float64) * (1 << (bits - 1))).astype(np.int64)
        assert (info["bits_per_sample"], info["channels"], info["samplerate"], info["total_samples"]) == (bits, 2, runs.rate, want.shape[0])
        assert info["md5"] == bytes(16)                                      # not computed: the samples never reached the host
        assert np.array_equal(pcm, want)
        assert all(s["wasted"] == 0 for d in frames for s in d["subframes"] if s["type"] != "CONSTANT")
        wide = wide or bool((pcm % 256 != 0).any())
        # fed back as an input, the device decoder restores exactly what read_wav gives for the WAV
        mix = runs.inst._device_mix_flac(fp, check_silent=False)
        assert mix is not None and np.array_equal(mix.cpu().numpy(), x)
    assert wide or bits == 16, "a 24-bit stream of v << 8 only"
    runs.inst.clear_gpu_cache()
    runs.inst.clear_file_specific_paths()


def test_flac_name_with_float_input_is_refused(runs, caplog):
    with caplog.at_level(logging.ERROR, logger=SC.log.name):
        got = runs.separate(runs.inputs["FLOAT"], "fast", fmt="FLAC")
    assert got["names"] and not any(os.path.exists(p) for p in got["paths"])
    assert got["how"] is None and got["left"] == {}
    assert any("FLAC holds no FLOAT samples" in r.getMessage() for r in caplog.records)
