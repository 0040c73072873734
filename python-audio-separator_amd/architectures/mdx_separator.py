"""MDXSeparator on the HIP engine: drop-in for audio_separator/separator/architectures/mdx_separator.py.

Same constructor (``common_config``, ``arch_config``), attributes, ``load_model`` / ``separate`` / ``demix`` /
``run_model`` / ``initialize_model_settings`` / ``initialize_mix`` contract, output naming and ``ValueError``s.
``ort.InferenceSession(model_path)`` (:108-133) is replaced by the ONNX reader + ``asx_net_*``; the array work of
``separate`` (:155-182) -- peak, in-place normalise, demix, ``* peak``, ``mix.T - compensate * primary`` -- is one C call
(``asx_separate``) and the writer's normalise / int16 / interleave another (``asx_pcm16``).
"""
from __future__ import annotations

import numpy as np

from ..common_separator import CommonSeparator
from ..mdx import MDXDemixer


class MDXSeparator(CommonSeparator):
    def __init__(self, common_config, arch_config):
        super().__init__(config=common_config)
        self._read_options(arch_config, (("segment_size", None), ("overlap", None), ("batch_size", 1), ("hop_length", None),
                                         ("enable_denoise", None)))
        self.logger.debug(f"MDX arch params: batch_size={self.batch_size}, segment_size={self.segment_size}, overlap={self.overlap}, "
                          f"hop_length={self.hop_length}, enable_denoise={self.enable_denoise}")
        md = self.model_data                                   # the hash-keyed model parameters (separator.py:786-803)
        self.compensate, self.dim_f, self.n_fft = md["compensate"], md["mdx_dim_f_set"], md["mdx_n_fft_scale_set"]
        self.dim_t = 2 ** md["mdx_dim_t_set"]
        self.config_yaml = md.get("config_yaml")
        # engine knob, not a reference option: chunks per device batch (results do not depend on it)
        self._max_batch = int(arch_config.get("asx_max_batch", 0))
        self._common, self._arch = dict(common_config), dict(arch_config)

        self.load_model()

        self.n_bins = self.trim = self.chunk_size = self.gen_size = 0      # filled by initialize_model_settings
        self.stft = None
        self._reset_file_state()

    def load_model(self):
        """mdx_separator.py:108-133.  ``common_config["asx_state_dict"]`` (a ConvTDFNet state_dict, optional, with
        ``asx_net_config``) bypasses the file for callers that hold the weights in memory."""
        common = dict(self._common)
        common["logger"] = self.logger
        self._dm = MDXDemixer(common, self._arch, state_dict=common.get("asx_state_dict"),
                              net_config=common.get("asx_net_config"), max_batch=self._max_batch)
        self.engine = self._dm.engine
        self.model_run = self._dm.engine.net_forward     # spek [B, 4, dim_f, dim_t] -> same (mdx_separator.py:123)

    def initialize_model_settings(self):
        """mdx_separator.py:205-228."""
        self._dm.initialize_model_settings()
        self.n_bins, self.trim = self._dm.n_bins, self._dm.trim
        self.chunk_size, self.gen_size, self.stft = self._dm.chunk_size, self._dm.gen_size, self._dm.stft

    def initialize_mix(self, mix, is_ckpt=False):
        """mdx_separator.py:230-291 (unused by demix in the reference as well): chunk tensor + pad, as numpy."""
        if mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got {mix.shape[0]} channels")
        self.initialize_model_settings()
        n = mix.shape[-1]
        if is_ckpt:
            pad = self.gen_size + self.trim - (n % self.gen_size)
            mixture = np.concatenate((np.zeros((2, self.trim), "float32"), mix, np.zeros((2, pad), "float32"),
                                      np.zeros((2, self.trim), "float32")), 1)
            waves = [mixture[:, i * self.gen_size: i * self.gen_size + self.chunk_size]
                     for i in range(mixture.shape[-1] // self.gen_size)]
        else:
            pad = self.gen_size - n % self.gen_size
            mix_p = np.concatenate((np.zeros((2, self.trim)), mix, np.zeros((2, pad)), np.zeros((2, self.trim))), 1)
            waves, i = [], 0
            while i < n + pad:
                waves.append(np.array(mix_p[:, i: i + self.chunk_size]))
                i += self.gen_size
        return np.asarray(waves, dtype=np.float32), pad

    def demix(self, mix, is_match_mix=False):
        """mdx_separator.py:293-412: float32 [2, N] -> [2, N]."""
        out = self._dm.demix(mix, is_match_mix=is_match_mix)
        self.n_bins, self.trim = self._dm.n_bins, self._dm.trim
        self.chunk_size, self.gen_size, self.stft = self._dm.chunk_size, self._dm.gen_size, self._dm.stft
        return out

    def run_model(self, mix, is_match_mix=False):
        """mdx_separator.py:414-450."""
        return self._dm.run_model(mix, is_match_mix=is_match_mix)

    def _device_stems(self):
        """The stems of the current file with every array in HBM (RIFF/WAVE input at the model's rate): data chunk -> pinned ->
        device -> asx_pcm_decode_dev -> asx_separate_dev.  Returns (primary, secondary), CUDA tensors [N, 2], or None when the
        file needs the host decoder or ``invert_using_spec`` the host path."""
        if self.invert_using_spec:
            return None
        mix = self._device_mix(self.audio_file_path)
        if mix is None:
            return None
        import torch
        t0 = self._now()
        self.initialize_model_settings()
        n = mix.shape[1]
        primary = torch.empty((n, 2), dtype=torch.float32, device=mix.device)
        secondary = torch.empty((n, 2), dtype=torch.float32, device=mix.device)
        self.engine.separate_dev(mix.data_ptr(), n, self.normalization_threshold, self.amplification_threshold, self.compensate,
                                 primary.data_ptr(), secondary.data_ptr(), stream=self._stream())
        self._tick("demix", t0)
        return primary, secondary

    def stems_dev(self, audio_file_path):
        """The stems ``separate(audio_file_path)`` would hand to write_audio, in its order (secondary first), left on the device:
        [(stem name, CUDA tensor [N, 2], "rows")]; honours ``output_single_stem``.  None when the file needs the host decoder
        (the condition under which ``_device_mix`` returns None).  Writes nothing."""
        self._begin_file(audio_file_path)
        stems = self._device_stems()
        if stems is None:
            return None
        primary, secondary = stems
        return [(name, t, "rows") for name, t in ((self.secondary_stem_name, secondary), (self.primary_stem_name, primary))
                if self._wanted(name)]

    def _separate_on_device(self, custom_output_names):
        """``_device_stems`` -> [host mirrors of the float stems, pinned, for ``primary_source`` / ``secondary_source``] ->
        asx_pcm16_rows_dev per written stem -> int16 back -> container.  The float stems are never uploaded again.  Returns
        None when the file needs the host decoder (the caller continues on the generic path)."""
        stems = self._device_stems()
        if stems is None:
            return None
        primary, secondary = stems
        t0 = self._now()
        if not isinstance(self.primary_source, np.ndarray):
            self.primary_source = self._host_stem(primary)
        if not isinstance(self.secondary_source, np.ndarray):
            self.secondary_source = self._host_stem(secondary)
        self._sync()                     # the host mirrors are complete before anyone can read primary_source / secondary_source
        self._tick("stems_d2h", t0)
        return self._emit_pair(custom_output_names)

    def separate(self, audio_file_path, custom_output_names=None):
        """mdx_separator.py:135-203."""
        self._begin_file(audio_file_path)
        files = self._separate_on_device(custom_output_names)
        if files is not None:
            return files
        mix = self.prepare_mix(self.audio_file_path)
        if mix.shape[0] != 2:
            msg = f"Expected a 2-channel audio signal, but got {mix.shape[0]} channels"
            self.logger.error(msg)
            raise ValueError(msg)
        mix = np.ascontiguousarray(mix, np.float32)
        self.initialize_model_settings()
        need_primary = not isinstance(self.primary_source, np.ndarray)
        need_secondary = not isinstance(self.secondary_source, np.ndarray)
        # peak / normalise(mix) in place / demix * peak / mix.T - compensate * primary (or invert_stem): MDXDemixer.separate_stems
        primary, secondary = self._dm.separate_stems(mix)
        if need_primary:
            self.primary_source = primary
        if need_secondary:
            self.secondary_source = secondary

        return self._emit_pair(custom_output_names)

    # ---- a batch of files in one pooled engine call -----------------------------------------------------------------
    _PER_FILE = ("audio_file_path", "audio_file_base", "input_bit_depth", "input_subtype", "_file_seconds")

    def _load_for_batch(self, path):
        """One file as ``separate`` would load it: (device mix [2, N] or None, host mix or None) -- the device decoder when the
        file allows it, else ``prepare_mix`` with the same refusals."""
        self._reset_file_state()
        self._begin_file(path)
        if not self.invert_using_spec:
            mix = self._device_mix(self.audio_file_path)
            if mix is not None:
                return mix, None
        mix = self.prepare_mix(self.audio_file_path)
        if mix.shape[0] != 2:
            msg = f"Expected a 2-channel audio signal, but got {mix.shape[0]} channels"
            self.logger.error(msg)
            raise ValueError(msg)
        return None, np.ascontiguousarray(mix, np.float32)

    def separate_many(self, paths, custom_output_names=None):
        """``separate`` for a list of files with ONE pooled engine call: every file is loaded as ``separate`` loads it, the
        chunks of all of them share the net passes (``asx_separate_batch_dev``), then each file's stems go through the same
        writer and naming code.  Returns one list of output names per input, in order; the files are byte-identical to those of
        ``separate(path)`` called per path.

        A file that cannot be used (unreadable, empty or silent, not stereo) fails alone, like the orchestrator's per-file
        ``try``: its entry in the result is an empty list, the exception is logged and kept in ``self.batch_errors[index]``;
        the other files are processed.  ``custom_output_names`` applies to every file, as it does in ``separate``."""
        import torch
        paths = list(paths)
        self.batch_errors = {}
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
        self.initialize_model_settings()
        if self.invert_using_spec:
            stems = self._dm.separate_stems_many([h for _, _, _, h in loaded])
        else:
            dev = self._torch_device()
            mixes = [d if d is not None else torch.from_numpy(h).to(dev) for _, _, d, h in loaded]
            prim = [torch.empty((m.shape[1], 2), dtype=torch.float32, device=dev) for m in mixes]
            sec = [torch.empty((m.shape[1], 2), dtype=torch.float32, device=dev) for m in mixes]
            self.engine.separate_batch_dev([(m.data_ptr(), p.data_ptr(), s.data_ptr(), m.shape[1]) for m, p, s in zip(mixes, prim, sec)],
                                           self.normalization_threshold, self.amplification_threshold, self.compensate,
                                           stream=self._stream())
            stems = list(zip(prim, sec))
        self._in_separate = True
        try:
            for (i, state, dev_mix, _), (primary, secondary) in zip(loaded, stems):
                self._reset_file_state()
                for k, v in state.items():
                    setattr(self, k, v)
                if isinstance(primary, np.ndarray):
                    self.primary_source, self.secondary_source = primary, secondary
                elif dev_mix is not None:                 # decoded on the device: the stems stay there for the writer, as in separate()
                    self.primary_source, self.secondary_source = self._host_stem(primary), self._host_stem(secondary)
                    self._sync()
                else:                                     # decoded on the host: host stems and the host writer, as in separate()
                    self.primary_source, self.secondary_source = primary.cpu().numpy(), secondary.cpu().numpy()
                try:
                    results[i] = self._emit_pair(custom_output_names)
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
