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
    def __init__(self, common_config, arch_config):
        super().__init__(config=common_config)
        self._read_options(arch_config, (("segment_size", "Default"), ("shifts", 2), ("overlap", 0.25), ("segments_enabled", True)))
        self.logger.debug(f"Demucs arch params: segment_size={self.segment_size}, segments_enabled={self.segments_enabled}, "
                          f"shifts={self.shifts}, overlap={self.overlap}")
        self.demucs_source_map = DEMUCS_4_SOURCE_MAPPER
        self.demucs_model_instance = None
        self._common, self._arch = dict(common_config), dict(arch_config)
        self._max_batch = int(arch_config.get("asx_max_batch", 0))
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

    def demix_demucs(self, mix):
        """demucs_separator.py:162-194: [2, N] -> [S, 2, N] with sources 0 / 1 swapped."""
        dm = self.load_model()
        dm.shifts, dm.overlap, dm.segments_enabled = self.shifts, self.overlap, self.segments_enabled
        out = dm.demix(np.ascontiguousarray(mix, np.float32))
        self.engine = dm.engine
        return out

    def _device_stems(self):
        """RIFF/WAVE input at the model's rate: data chunk -> pinned -> HBM -> asx_pcm_decode_dev -> the demix (single model or
        bag) -> stems [S, 2, N] that STAY in HBM.  None when the file needs the host decoder or the configuration the host
        combine."""
        dm = self.load_model()                      # binds self.engine, which the device decode needs
        mix_d = self._device_mix(self.audio_file_path)
        if mix_d is None:
            return None
        t0 = self._now()
        dm.shifts, dm.overlap, dm.segments_enabled = self.shifts, self.overlap, self.segments_enabled
        out_d = dm.demix_dev(mix_d) if hasattr(dm, "demix_dev") else None
        self.engine = dm.engine
        if out_d is not None:
            self._tick("demix", t0)
        return out_d

    def _source_map(self, n_sources):
        self.demucs_source_map = {2: DEMUCS_2_SOURCE_MAPPER, 6: DEMUCS_6_SOURCE_MAPPER}.get(n_sources, DEMUCS_4_SOURCE_MAPPER)
        return self.demucs_source_map

    def _single_stem_skips(self, stem_name):
        return self.output_single_stem is not None and stem_name.lower() != self.output_single_stem.lower()

    def stems_dev(self, audio_file_path):
        """The stems ``separate(audio_file_path)`` would hand to write_audio, in the order of the source map, left on the device:
        [(stem name, CUDA tensor [2, N], "planar")]; honours ``output_single_stem``.  None when the file needs the host decoder
        or the configuration the host combine.  Writes nothing."""
        self._begin_file(audio_file_path)
        out_d = self._device_stems()
        if out_d is None:
            return None
        return [(name, out_d[index], "planar") for name, index in self._source_map(len(out_d)).items()
                if not self._single_stem_skips(name)]

    def _demix_on_device(self):
        """``_device_stems``; ``source`` is the pinned host mirror of the stems and every ``source[i].T`` view handed to
        write_audio is registered against its device tensor, so the int16 pass runs on the device (asx_pcm16_dev) without a
        second upload.  (None, None) when there is no device-resident path for this file."""
        out_d = self._device_stems()
        if out_d is None:
            return None, None
        t0 = self._now()
        source, views = self._host_planar_stems(out_d)
        self._sync()
        self._tick("stems_d2h", t0)
        return source, views

    def separate(self, audio_file_path, custom_output_names=None):
        """demucs_separator.py:83-160."""
        self._begin_file(audio_file_path)
        source, views = self._demix_on_device()
        if source is None:
            mix = self.prepare_mix(self.audio_file_path)
            self.load_model()
            source = self.demix_demucs(mix)
            self.clear_gpu_cache()

        return self._emit_stems(source, views, custom_output_names)

    def _emit_stems(self, source, views, custom_output_names):
        files = []
        for stem_name, index in self._source_map(len(source)).items():
            if self._single_stem_skips(stem_name):
                self.logger.debug(f"{stem_name}: not written (output_single_stem = {self.output_single_stem})")
                continue
            path = self.get_stem_output_path(stem_name, custom_output_names)
            self.final_process(path, views[index] if views is not None else source[index].T, stem_name)
            files.append(path)
        return files

    # ---- a batch of files in one pooled engine call -----------------------------------------------------------------
    _PER_FILE = ("audio_file_path", "audio_file_base", "input_bit_depth", "input_subtype", "_file_seconds")

    def _load_for_batch(self, path):
        """One file as ``separate`` would load it: (device mix [2, N] or None, host mix or None)."""
        self._reset_file_state()
        self._begin_file(path)
        mix = self._device_mix(self.audio_file_path)
        if mix is not None:
            return mix, None
        mix = np.ascontiguousarray(self.prepare_mix(self.audio_file_path), np.float32)
        if mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
        return None, mix

    def separate_many(self, paths, custom_output_names=None):
        """``separate`` for a list of files with ONE pooled demix (``DemucsDemixer.demix_many_dev``: the segments of all files
        share the forwards), then each file's stems go through the same writer and naming code.  Returns one list of output
        names per input, in order.  The shift offsets are drawn in file order, so under one ``random.seed`` the files equal
        those of ``separate(path)`` called per path.

        A file that cannot be used fails alone: its entry is an empty list, the exception is logged and kept in
        ``self.batch_errors[index]``.  ``custom_output_names`` applies to every file, as it does in ``separate``."""
        from ..demucs import _cuda_ready
        paths = list(paths)
        self.batch_errors = {}
        dm = self.load_model()
        dm.shifts, dm.overlap, dm.segments_enabled = self.shifts, self.overlap, self.segments_enabled
        loaded = []                                       # (index, per-file state, device mix, host mix)
        for i, path in enumerate(paths):
            try:
                dev_mix, host_mix = self._load_for_batch(path)
            except Exception as e:                        # this file only
                self.logger.error(f"{path}: {e}")
                self.batch_errors[i] = e
                continue
            loaded.append((i, {k: getattr(self, k) for k in self._PER_FILE}, dev_mix, host_mix))
        results = [[] for _ in paths]
        if not loaded:
            self._reset_file_state()
            return results
        on_device = self.segments_enabled and _cuda_ready()
        if on_device:
            import torch
            dev = torch.device("cuda", dm.device)
            stems = dm.demix_many_dev([d if d is not None else torch.from_numpy(h).to(dev) for _, _, d, h in loaded])
        else:                                             # segments_enabled=False windows on the host; so does an engine double
            stems = dm.demix_many([h if h is not None else d.cpu().numpy() for _, _, d, h in loaded])
        self.engine = dm.engine
        self._in_separate = True
        try:
            for (i, state, dev_mix, _), out in zip(loaded, stems):
                self._reset_file_state()
                for k, v in state.items():
                    setattr(self, k, v)
                try:
                    if on_device and dev_mix is not None:   # decoded on the device: the stems stay there for the writer, as in separate()
                        source, views = self._host_planar_stems(out)
                        self._sync()
                    else:
                        source, views = (out.cpu().numpy() if on_device else out), None
                    results[i] = self._emit_stems(source, views, custom_output_names)
                except Exception as e:
                    self.logger.error(f"{state['audio_file_path']}: {e}")
                    self.batch_errors[i] = e
        except BaseException:
            self._in_separate = False
            self._drain_writes(raise_errors=False)
            raise
        self._in_separate = False
        self._drain_writes()
        return results
