"""DemucsSeparator on the HIP engine: drop-in for audio_separator/separator/architectures/demucs_separator.py.

Same constructor, ``separate`` / ``demix_demucs`` contract, source maps and output naming.  The model package
(``.th`` + bag ``.yaml``, read without importing or executing any Demucs code -- model_files.py) is loaded once and
kept resident instead of being re-read for every file (:119-124); ``apply_model`` with its shift trick, segment split
and triangular fold, the HTDemucs / HDemucs forward and the standardise / de-standardise / stem swap of ``demix_demucs``
(:162-194) are ``asx_ht_demix`` / ``asx_hd_demix``.
"""
from __future__ import annotations


import numpy as np

from ..common_separator import CommonSeparator
from ..demucs import DemucsDemixer

DEMUCS_4_SOURCE = ["drums", "bass", "other", "vocals"]
DEMUCS_2_SOURCE_MAPPER = {CommonSeparator.INST_STEM: 0, CommonSeparator.VOCAL_STEM: 1}
DEMUCS_4_SOURCE_MAPPER = {CommonSeparator.BASS_STEM: 0, CommonSeparator.DRUM_STEM: 1, CommonSeparator.OTHER_STEM: 2,
                          CommonSeparator.VOCAL_STEM: 3}
DEMUCS_6_SOURCE_MAPPER = {CommonSeparator.BASS_STEM: 0, CommonSeparator.DRUM_STEM: 1, CommonSeparator.OTHER_STEM: 2,
                          CommonSeparator.VOCAL_STEM: 3, CommonSeparator.GUITAR_STEM: 4, CommonSeparator.PIANO_STEM: 5}


class DemucsSeparator(CommonSeparator):
    _autocast_refusal = CommonSeparator._AUTOCAST_ONLY_ROFORMER
    _complement_rate_refusal = "every stem is an output of the model; none of them is formed as the mix minus another stem"

    def __init__(self, common_config, arch_config):
        super().__init__(config=common_config)
        self._read_options(arch_config, (("segment_size", "Default"), ("shifts", 2), ("overlap", 0.25), ("segments_enabled", True)))
        self.logger.debug(f"Demucs arch params: segment_size={self.segment_size}, segments_enabled={self.segments_enabled}, "
                          f"shifts={self.shifts}, overlap={self.overlap}")
        self.demucs_source_map = DEMUCS_4_SOURCE_MAPPER
        self.demucs_model_instance = None
        self._keep_configs(common_config, arch_config)
        self.logger.info("Demucs plugin ready (the model package is read at the first separate())")

    def load_model(self):
        """demucs_separator.py:119-124 (get_demucs_model + demucs_segments + .to(device).eval()), done once."""
        if self.demucs_model_instance is None:
            common = dict(self._common)
            common["logger"] = self.logger
            self.demucs_model_instance = DemucsDemixer(common, self._arch, models=common.get("asx_models"),
                                                       weights=common.get("asx_weights"), max_batch=self._max_batch)
            self.demucs_model_instance._load(0)
            self.engine = self.demucs_model_instance.engine
        return self.demucs_model_instance

    def _prepare_model(self):
        """The resident model with this instance's options; binds ``self.engine``, which the device decode needs, so it runs
        before a file is loaded."""
        dm = self.load_model()
        dm.shifts, dm.overlap, dm.segments_enabled = self.shifts, self.overlap, self.segments_enabled
        return dm

    def demix_demucs(self, mix):
        """demucs_separator.py:162-194: [2, N] -> [S, 2, N] with sources 0 / 1 swapped."""
        dm = self._prepare_model()
        out = dm.demix(np.ascontiguousarray(mix, np.float32))
        self.engine = dm.engine
        return out

    def _require_stereo(self, mix):
        if mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")

    def _device_stems(self, dm, mix_d):
        """A mix decoded on the device -> the demix (single model or bag) -> stems [S, 2, N] that STAY in HBM.  None when the
        configuration needs the host combine."""
        t0 = self._now()
        out_d = dm.demix_dev(mix_d) if hasattr(dm, "demix_dev") else None      # (an engine double has no device calls)
        self.engine = dm.engine
        if out_d is not None:
            self._tick("demix", t0)
        return out_d

    def _source_map(self, n_sources):
        self.demucs_source_map = {2: DEMUCS_2_SOURCE_MAPPER, 6: DEMUCS_6_SOURCE_MAPPER}.get(n_sources, DEMUCS_4_SOURCE_MAPPER)
        return self.demucs_source_map

    def _single_stem_skips(self, stem_name):
        # ``is not None`` as the reference's Demucs plugin has it; CommonSeparator._wanted (the MDX family) tests truthiness, so
        # the two differ for output_single_stem == "" and stay apart
        return self.output_single_stem is not None and stem_name.lower() != self.output_single_stem.lower()

    def _written_stems(self, n_sources):
        """(stem name, row of the stems) of what gets written, in the order of the source map."""
        for stem_name, index in self._source_map(n_sources).items():
            if self._single_stem_skips(stem_name):
                self.logger.debug(f"{stem_name}: not written (output_single_stem = {self.output_single_stem})")
            else:
                yield stem_name, index

    def stems_dev(self, audio_file_path):
        """The stems ``separate(audio_file_path)`` would hand to write_audio, in the order of the source map, left on the device:
        [(stem name, CUDA tensor [2, N], "planar")]; honours ``output_single_stem``.  None when the file needs the host decoder
        or the configuration the host combine.  Writes nothing."""
        self._begin_file(audio_file_path)
        dm = self._prepare_model()
        mix_d = self._device_decode(self.audio_file_path)
        out_d = self._device_stems(dm, mix_d) if mix_d is not None else None
        return self._stems_of(out_d)

    def _stems_of(self, out_d):
        """Stems [S, 2, N] in HBM -> the list ``stems_dev`` returns (None: the configuration combined on the host)."""
        if out_d is None or isinstance(out_d, np.ndarray):
            return None
        return [(name, out_d[index], "planar") for name, index in self._written_stems(len(out_d))]

    def _emit_file(self, out, on_device, custom_output_names):
        """Stems [S, 2, N] of the current file -> its output files.  Decoded and demixed on the device: the source is the pinned
        host mirror of the stems and every ``source[i].T`` view handed to write_audio is registered against its device tensor, so
        the int16 pass runs on the device (asx_pcm16_dev) without a second upload.  Else host stems and the host writer."""
        t0 = self._now()
        if on_device and not isinstance(out, np.ndarray):
            _, views = self._host_planar_stems(out)
            self._sync()
            self._tick("stems_d2h", t0)
        else:
            views = [stem.T for stem in self._to_host(out)]
        files = []
        for stem_name, index in self._written_stems(len(views)):
            path = self.get_stem_output_path(stem_name, custom_output_names)
            self.final_process(path, views[index], stem_name)
            files.append(path)
        return files

    def separate(self, audio_file_path, custom_output_names=None):
        """demucs_separator.py:83-160."""
        self._begin_file(audio_file_path)
        dm = self._prepare_model()
        dev_mix, host_mix = self._load_mix(self.audio_file_path)
        out = self._device_stems(dm, dev_mix) if dev_mix is not None else None
        on_device = out is not None
        if not on_device:
            # (a file the device decoded under a configuration that combines on the host is decoded again, by prepare_mix)
            out = self.demix_demucs(host_mix if host_mix is not None else self._host_mix(self.audio_file_path))
            self.clear_gpu_cache()
        return self._emit_file(out, on_device, custom_output_names)

    # ---- a batch of files: the hooks of CommonSeparator._separate_many ------------------------------------------------------
    # The shift offsets are drawn in file order, so under one ``random.seed`` the files equal those of ``separate(path)`` called per path.
    separate_many = CommonSeparator._separate_many
    stems_dev_many = CommonSeparator._stems_dev_many

    def _pooled_stems(self, mixes):
        """``DemucsDemixer.demix_many_dev``: the segments of all files share the forwards."""
        from ..demucs import _cuda_ready
        dm = self.demucs_model_instance
        if self.segments_enabled and _cuda_ready():
            stems = dm.demix_many_dev(self._device_mixes(mixes))
        else:                                             # segments_enabled=False windows on the host; so does an engine double
            stems = dm.demix_many([h if h is not None else self._to_host(d) for d, h in mixes])
        self.engine = dm.engine
        return stems
