"""VRSeparator on the HIP engine: drop-in for audio_separator/separator/architectures/vr_separator.py.

Same constructor, attributes and ``separate`` contract (:115-253).  ``loading_mix`` / ``inference_vr`` / ``spec_to_wav``
and the spec_utils functions under them are one C call (``asx_vr_separate``, vr.py:VRDemixer); the network is built and
the ``.pth`` read once, at the first file, instead of at every ``separate`` (:158-178).

Resampler (vr.py ``resolve_res_type``): like the reference, the *synthesis* chain runs libsamplerate's ``sinc_fastest``
everywhere except macOS on ARM, where it runs ``polyphase`` (uvr_lib_v5/spec_utils.py:33-38), and the analysis chain runs each
band's own ``res_type``.  ``sinc_fastest`` is the library's published algorithm on a regenerated Kaiser-sinc table -- the
library's own table cannot be had here (INTEGRATION.md "VR resampler": parity unpinned for this converter, measured bounds
there); ``arch_config["asx_res_type"]`` = "polyphase" | "sinc_fastest" overrides the platform rule.  A warning is logged once
when a band asks for a converter the engine serves with the polyphase filter instead (``sinc_medium``, ``sinc_best``,
``kaiser_*`` -- in the shipped parameter files only top bands carry those, where they matter for non-44.1 kHz input files
decoded on the host).
"""
from __future__ import annotations

import math
import os

import numpy as np

from .. import audio_io
from ..common_separator import CommonSeparator
from ..model_files import read_state_dict
from ..vr import NN_ARCH_SIZES, VR_5_1, VRDemixer, load_model_params, reference_params_dir, reference_wav_resolution, resolve_res_type  # noqa: F401


class VRSeparator(CommonSeparator):
    # ``asx_input_resample`` = "device" does not reach this plugin: the reference decodes a VR input with the top band's own res_type
    # (vr_separator.py:255-291), not with librosa.load's soxr_hq, so a file at another rate keeps going to ``_host_mix``
    _resamples_input_files = False
    # for the same reason the way back is out of scope here: this plugin brings a file at another rate in on the host, with the band's own
    # res_type, and a writer-side conversion would have to answer to that converter
    _output_rate_refusal = ("its inputs at other rates are converted on the host with the band's own res_type, which the writer-side "
                            "converter does not mirror (a follow-up); leave asx_output_rate at 'model'")
    _complement_rate_refusal = "this plugin writes every stem at the model's rate (it refuses asx_output_rate='input')"
    _autocast_refusal = CommonSeparator._AUTOCAST_ONLY_ROFORMER

    def __init__(self, common_config, arch_config: dict):
        super().__init__(config=common_config)
        self.model_capacity = 32, 128
        self.is_vr_51_model = False
        if "nout" in self.model_data.keys() and "nout_lstm" in self.model_data.keys():
            self.model_capacity = self.model_data["nout"], self.model_data["nout_lstm"]
            self.is_vr_51_model = True
        params_dir = common_config.get("vr_params_dir") or reference_params_dir()
        self.model_params_path = os.path.join(params_dir or "", f"{self.model_data['vr_model_param']}.json")
        self.model_params = load_model_params(self.model_params_path)

        self._read_options(arch_config, (("enable_tta", False), ("enable_post_process", False), ("post_process_threshold", 0.2),
                                         ("batch_size", 1), ("window_size", 512), ("high_end_process", False)))
        self.input_high_end_h = None
        self.input_high_end = None
        self.aggression = float(int(arch_config.get("aggression", 5)) / 100)
        self.aggressiveness = {"value": self.aggression, "split_bin": self.model_params["band"][1]["crop_stop"],
                               "aggr_correction": self.model_params.get("aggr_correction")}
        self.model_samplerate = self.model_params["sr"]
        self.res_type = resolve_res_type(arch_config.get("asx_res_type"))
        self._keep_configs(common_config, arch_config)
        self._dm = None
        self.model_run = None
        self.logger.debug(f"VR arch params: enable_tta={self.enable_tta}, enable_post_process={self.enable_post_process}, "
                          f"post_process_threshold={self.post_process_threshold}, batch_size={self.batch_size}, "
                          f"window_size={self.window_size}, high_end_process={self.high_end_process}, aggression={self.aggression}")
        self.logger.info(f"VR plugin ready ({self.model_data['vr_model_param']}, {'5.1' if self.is_vr_51_model else '5.0'} net on the HIP engine)")

    def _warn_resampler(self):
        bands = self.model_params["band"]
        lower = {str(bands[d].get("res_type")) for d in bands if d != max(bands)}     # converters loading_mix really runs
        foreign = sorted(w for w in lower if w not in ("polyphase", "sinc_fastest", "None"))
        if foreign:
            self.logger.warning(f"VR analysis resampling: band entries ask for {foreign} (libsamplerate / resampy); this engine "
                                "serves them with the polyphase filter (INTEGRATION.md, 'VR resampler').")

    def load_model(self):
        """vr_separator.py:158-178: architecture size from the file size, CascadedASPPNet / CascadedNet, load_state_dict."""
        if self._dm is not None:
            return self._dm
        state_dict = self._common.get("asx_state_dict")
        if state_dict is None:
            model_size = math.ceil(os.stat(self.model_path).st_size / 1024)
            nn_arch_size = min(NN_ARCH_SIZES, key=lambda x: abs(x - model_size))
            state_dict = read_state_dict(self.model_path)
        else:
            nn_arch_size = self._common["asx_nn_arch_size"]
        nn_arch_size = self._common.get("asx_nn_arch_size", nn_arch_size)
        if nn_arch_size in VR_5_1 or self.is_vr_51_model:
            self.is_vr_51_model = True
        common = dict(self._common)
        common.update(model_params=self.model_params, primary_stem_name=self.primary_stem_name, logger=self.logger)
        self._dm = VRDemixer(common, self._arch, state_dict, nn_arch_size, capacity=self._common.get("asx_capacity"),
                             max_batch=self._max_batch)
        self.engine = self._dm.engine
        self.model_run = self._dm.engine.vr_forward
        self._warn_resampler()
        return self._dm

    def _prepare_model(self):
        """What ``separate`` does before a sample is touched, apart from the per-file state (vr_separator.py:158-178 and the
        ``output_single_stem`` check): the resident model -- which binds ``self.engine``, needed by the device decode -- and a
        single-stem name the model knows."""
        dm = self.load_model()
        if self.output_single_stem and self.output_single_stem.lower() not in (self.primary_stem_name.lower(),
                                                                               self.secondary_stem_name.lower()):
            self.logger.warning(f"output_single_stem = '{self.output_single_stem}' names neither '{self.primary_stem_name}' nor "
                                f"'{self.secondary_stem_name}' (model {self.model_name}): ignored, both stems are written")
            self.output_single_stem = None
        return dm

    def _begin_vr_file(self, audio_file_path):
        """Per-file state and the model.  Returns (demixer, want primary, want secondary)."""
        self._reset_file_state()
        self._begin_file(audio_file_path)
        dm = self._prepare_model()
        return dm, self._wanted(self.primary_stem_name), self._wanted(self.secondary_stem_name)

    # what a file leaves for the writer here, on top of the base class's list: VR records the input's sample format itself
    _PER_FILE = CommonSeparator._PER_FILE + ("wav_subtype", "input_audio_subtype")

    def _probe_vr_format(self, audio_file_path):
        """vr_separator.py:115-156: the input's sample format for the writer.  A mix handed in through the door of CommonSeparator brings
        what this probe would have found in its file."""
        injected = self._injected_for(audio_file_path)
        if injected is not None and "wav_subtype" in injected[1]:
            state = injected[1]
            self.wav_subtype, self.input_audio_subtype, self.input_bit_depth = state["wav_subtype"], state["input_audio_subtype"], state["input_bit_depth"]
            self.input_subtype = None
            return
        try:
            self.input_audio_subtype = audio_io.info(audio_file_path)["subtype"]
            if "24" in self.input_audio_subtype:
                self.wav_subtype, self.input_bit_depth = "PCM_24", 24
            elif "32" in self.input_audio_subtype:
                self.wav_subtype, self.input_bit_depth = "PCM_32", 32
            else:
                self.wav_subtype, self.input_bit_depth = "PCM_16", 16
        except Exception as e:
            self.logger.warning(f"{audio_file_path}: no container info ({e}); stems will be written as PCM_16")
            self.wav_subtype, self.input_audio_subtype, self.input_bit_depth = "PCM_16", None, 16
        # the reference's VR path never goes through prepare_mix, so input_subtype stays None and the soundfile writer picks
        # PCM_16 / 24 / 32 from input_bit_depth (common_separator.py:390-402); keep that
        self.input_subtype = None

    def _takes_device_mix(self) -> bool:
        bands = self.model_params["band"]
        return bands[len(bands)]["sr"] == self.sample_rate and self.model_samplerate == 44100

    def _device_decode(self, path):
        """Device-resident decode (RIFF/WAVE at the top band's rate, which is also the rate the stems are written at).  None
        when the file needs the host decoder.  A silent file is not refused: the reference's VR path has no such check."""
        if not self._takes_device_mix():
            return None
        # _device_mix records prepare_mix's fields; VR keeps its own (input_subtype None), so they are restored around it
        keep = (self.input_subtype, self.input_bit_depth)
        wave_d = self._device_mix(path, check_silent=False)
        self.input_subtype, self.input_bit_depth = keep
        return wave_d

    def _host_mix(self, path):
        """loading_mix (:255-291): the top band is the file decoded at the band's rate, mono duplicated; never ``prepare_mix``."""
        bands = self.model_params["band"]
        wave, _ = audio_io.load(path, sr=bands[len(bands)]["sr"], mono=False)
        if wave.ndim == 1:
            wave = np.asarray([wave, wave])
        return np.ascontiguousarray(wave, np.float32)

    def _load_mix(self, path):
        """One input file as the top band's wave [2, N]: (CUDA tensor, None) or (None, float32 array), after recording the
        input's sample format the way this plugin does."""
        self._probe_vr_format(path)
        return super()._load_mix(path)

    def _check_loaded(self, dev_mix, host_mix):
        """A wave too short for the model must not reach the pooled call, which would reject the whole pool."""
        n = (dev_mix if dev_mix is not None else host_mix).shape[1]
        frames, _ = self.engine.vr_plan(n)
        if frames < 2:
            raise ValueError(f"input too short: {n} samples make {frames} frame(s), the model needs 2")

    def stems_dev(self, audio_file_path):
        """The stems ``separate(audio_file_path)`` would hand to write_audio, primary first, left on the device:
        [(stem name, CUDA tensor [2, N'], "planar")]; honours ``output_single_stem``.  None when the file needs the host
        decoder.  Writes nothing."""
        dm, want_p, want_s = self._begin_vr_file(audio_file_path)
        self._probe_vr_format(audio_file_path)
        wave_d = self._device_decode(audio_file_path)
        if wave_d is None:
            return None
        t0 = self._now()
        stems_d = dm.separate_stems_dev(wave_d)
        self._tick("demix", t0)
        return self._stems_of(stems_d)

    def _stems_of(self, stems_d):
        """One CUDA tensor [2 (primary, secondary), 2, N'] -> the list ``stems_dev`` returns."""
        return [(name, stems_d[i], "planar") for i, name in enumerate((self.primary_stem_name, self.secondary_stem_name)) if self._wanted(name)]

    def _emit_file(self, stems, on_device, custom_output_names):
        """The stems of the current file -> its output files, primary first (vr_separator.py:211-246), unlike the MDX family.
        ``stems``: one CUDA tensor [2 (primary, secondary), 2, N'] -- mirrored into pinned host memory with every ``stems[i].T``
        view registered against its device tensor when the file was decoded on the device, so the int16 pass runs there; brought
        to the host otherwise -- or the pair of host arrays [N', 2] (None = not wanted) of ``VRDemixer.separate_stems``."""
        if not isinstance(stems, (tuple, list)):
            if on_device:
                t0 = self._now()
                _, stems = self._host_planar_stems(stems)
                self._sync()
                self._tick("stems_d2h", t0)
            else:
                stems = [stem.T for stem in self._to_host(stems)]
        files = []
        for which, name, stem in (("primary", self.primary_stem_name, stems[0]), ("secondary", self.secondary_stem_name, stems[1])):
            if self._wanted(name):
                source = self._to_44100(stem)
                setattr(self, f"{which}_source", source)
                setattr(self, f"{which}_stem_output_path", self._emit_stem(name, source, custom_output_names, files))
        return files

    def separate(self, audio_file_path, custom_output_names=None):
        """vr_separator.py:115-253."""
        dm, want_p, want_s = self._begin_vr_file(audio_file_path)
        dev_mix, host_mix = self._load_mix(audio_file_path)
        if dev_mix is not None:
            t0 = self._now()
            stems = dm.separate_stems_dev(dev_mix)
            self._tick("demix", t0)
        else:
            stems = dm.separate_stems(host_mix, want_primary=want_p, want_secondary=want_s)
        return self._emit_file(stems, dev_mix is not None, custom_output_names)

    # ---- a batch of files: the hooks of CommonSeparator._separate_many ------------------------------------------------------
    separate_many = CommonSeparator._separate_many
    stems_dev_many = CommonSeparator._stems_dev_many

    def _pooled_stems(self, mixes):
        """``VRDemixer.separate_stems_many_dev``: the patches of all files share the net passes; a stem ``output_single_stem``
        leaves out is not synthesised."""
        return self._dm.separate_stems_many_dev(self._device_mixes(mixes), want_primary=self._wanted(self.primary_stem_name),
                                                want_secondary=self._wanted(self.secondary_stem_name))

    def _to_44100(self, stem):
        """vr_separator.py:218-220, :238-240: models trained at another rate are brought back with librosa.resample's
        default converter (soxr_hq) -- a host library the reference depends on; it is used when present."""
        if self.model_samplerate == 44100:
            return stem
        librosa = audio_io._optional("librosa")
        if librosa is not None and hasattr(librosa, "resample"):
            return librosa.resample(stem.T, orig_sr=self.model_samplerate, target_sr=44100).T
        # no librosa in this environment (the reference itself could not run here): the engine's libsamplerate-style converter
        # stands in for soxr_hq -- same band limit to well below 1e-3, not the same filter
        if not getattr(self, "_warned_soxr", False):
            self._warned_soxr = True
            self.logger.warning(f"model sample rate {self.model_samplerate} != 44100 and librosa is not installed: the final resample "
                                "uses the engine's sinc_fastest converter instead of librosa's default soxr_hq")
        ratio = float(44100) / self.model_samplerate
        return np.ascontiguousarray(self.engine.resample_sinc(np.ascontiguousarray(np.asarray(stem, np.float32).T), ratio).T)
