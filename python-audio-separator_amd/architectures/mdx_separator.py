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
    _autocast_refusal = CommonSeparator._AUTOCAST_ONLY_ROFORMER

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
        self._keep_configs(common_config, arch_config)
        if self.asx_complement_rate == "input" and self.invert_using_spec:
            raise ValueError("asx_complement_rate='input' is not supported with invert_using_spec: the secondary stem is then a spectral "
                             "inversion, not the difference mix - compensate * primary")

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

    # ---- one file: load (base ``_load_mix``), stems, ``_emit_file`` ---------------------------------------------------------
    def _require_stereo(self, mix):
        if mix.shape[0] != 2:
            msg = f"Expected a 2-channel audio signal, but got {mix.shape[0]} channels"
            self.logger.error(msg)
            raise ValueError(msg)

    def _complement_stem_name(self):
        """The secondary stem, ``mix - compensate * primary`` -- unless ``invert_using_spec`` makes it a spectral inversion."""
        return None if self.invert_using_spec else self.secondary_stem_name

    def _device_stems(self, mix):
        """The stems of a mix decoded on the device (CUDA tensor [2, N]) with every array in HBM: asx_separate_dev.  Returns
        (primary, secondary), CUDA tensors [N, 2].  ``invert_using_spec``: the steps of MDXDemixer.separate_stems on the same stream --
        the match-mix demix of the normalised mix, then asx_invert_stem_dev over the rows primary scaled by ``compensate``; the
        secondary stem is [1024 * (N // 1024), 2], shorter than the primary as on the host path."""
        import torch
        t0 = self._now()
        self.initialize_model_settings()
        n = mix.shape[1]
        primary = torch.empty((n, 2), dtype=torch.float32, device=mix.device)
        secondary = torch.empty((n, 2), dtype=torch.float32, device=mix.device)
        self.engine.separate_dev(mix.data_ptr(), n, self.normalization_threshold, self.amplification_threshold, self.compensate,
                                 primary.data_ptr(), secondary.data_ptr(), stream=self._stream())
        if self.invert_using_spec:
            raw = secondary.view(2, n)                    # mix.T - compensate * primary is not used: its buffer takes the match-mix demix
            self.engine.demix_dev(mix.data_ptr(), n, raw.data_ptr(), is_match_mix=True, stream=self._stream())
            t0 = self._tick("demix", t0)
            n_out = 1024 * (n // 1024)
            secondary = torch.empty((n_out, 2), dtype=torch.float32, device=mix.device)
            self.engine.invert_stem_dev(raw.data_ptr(), primary.data_ptr(), n, "rows", self.compensate, secondary.data_ptr(), n_out,
                                        stream=self._stream())
            self._tick("invert", t0)
            return primary, secondary
        self._tick("demix", t0)
        return primary, secondary

    def stems_dev(self, audio_file_path):
        """The stems ``separate(audio_file_path)`` would hand to write_audio, in its order (secondary first), left on the device:
        [(stem name, CUDA tensor [N, 2], "rows")]; honours ``output_single_stem``.  None when the file needs the host decoder
        (the condition under which ``_device_decode`` returns None).  Writes nothing.  With ``invert_using_spec`` the secondary stem
        has 1024 * (N // 1024) rows, and is not in the list below 1024 samples."""
        self._begin_file(audio_file_path)
        self._stems_only = True                           # (nothing is written: asx_complement_rate has no use for the file's mix)
        try:
            mix = self._device_decode(self.audio_file_path)
        finally:
            self._stems_only = False
        if mix is None:
            return None
        return self._stems_of(self._device_stems(mix))

    def _stems_of(self, stems):
        """(primary, secondary) CUDA tensors [N, 2] -> the list ``stems_dev`` returns.  An empty stem (``invert_using_spec`` on fewer
        than 1024 samples) is left out: ``separate`` writes no file for it, so an ensemble has nothing of it to combine."""
        stems = dict(zip(("primary", "secondary"), stems))
        return [(name, stems[which], "rows") for name, which in self._wanted_pair() if stems[which].shape[0]]

    def _emit_file(self, stems, on_device, custom_output_names):
        """(primary, secondary) of the current file -> its output files.  Decoded on the device: the float stems stay there, the
        sources are their pinned host mirrors and asx_pcm16_rows_dev quantises each written stem without a second upload.
        Decoded on the host: host stems and the host writer."""
        t0 = self._now()
        # (an empty stem -- invert_using_spec on fewer than 1024 samples -- has nothing to quantise on the device: the writer's "nothing
        # to write" branch gets a plain empty array, as on the host path)
        mirror = (lambda stem: self._host_stem(stem) if stem.shape[0] else self._to_host(stem)) if on_device else self._to_host
        # a primary_source / secondary_source set before separate() is honoured: unlike MDXC and VR, separate() here does not
        # reset the file state first (separate_many does, per file)
        made = 0
        for which, stem in zip(("primary", "secondary"), stems):
            if not isinstance(getattr(self, f"{which}_source"), np.ndarray):
                setattr(self, f"{which}_source", mirror(stem))
                made += 1
        # asx_complement_rate = "input": the secondary file is written from s * (the file's mix) - compensate * (the converted primary)
        self._register_complement(self.secondary_source if made == 2 else None, self.primary_source, self.compensate, False,
                                  model_wanted=self._wanted(self.primary_stem_name))
        if on_device:
            self._sync()                 # the host mirrors are complete before anyone can read primary_source / secondary_source
            self._tick("stems_d2h", t0)
        return self._emit_pair(custom_output_names)

    def separate(self, audio_file_path, custom_output_names=None):
        """mdx_separator.py:135-203."""
        self._begin_file(audio_file_path)
        dev_mix, host_mix = self._load_mix(self.audio_file_path)
        self._mix_scale = self._mix_factor(dev_mix, host_mix)      # (before the stem call normalises the mix in place)
        if dev_mix is not None:
            stems = self._device_stems(dev_mix)
        else:
            self.initialize_model_settings()
            # peak / normalise(mix) in place / demix * peak / mix.T - compensate * primary (or invert_stem): MDXDemixer.separate_stems
            stems = self._dm.separate_stems(host_mix)
        return self._emit_file(stems, dev_mix is not None, custom_output_names)

    # ---- a batch of files: the hooks of CommonSeparator._separate_many ------------------------------------------------------
    separate_many = CommonSeparator._separate_many
    stems_dev_many = CommonSeparator._stems_dev_many

    def _pooled_stems(self, mixes):
        """asx_separate_batch_dev: the chunks of all files share the net passes."""
        self.initialize_model_settings()                  # after the files are loaded, where separate() runs it
        if self.invert_using_spec and not self._fast_file_path_enabled():      # every file was decoded on the host: the host arrays' path
            return self._dm.separate_stems_many([h for _, h in mixes])
        import torch
        mixes = self._device_mixes(mixes)
        self._pool_mix_scales = [self._mix_factor(m, None, kept) for m, kept in zip(mixes, self._pool_kept)]
        prim = [torch.empty((m.shape[1], 2), dtype=torch.float32, device=m.device) for m in mixes]
        sec = [torch.empty_like(p) for p in prim]
        self.engine.separate_batch_dev([(m.data_ptr(), p.data_ptr(), s.data_ptr(), m.shape[1]) for m, p, s in zip(mixes, prim, sec)],
                                       self.normalization_threshold, self.amplification_threshold, self.compensate,
                                       stream=self._stream())
        if self.invert_using_spec:
            # MDXDemixer.separate_stems_many on the device: one pooled match-mix demix of the normalised mixes (into the buffers of the
            # unused mix.T - compensate * primary), one pooled invert_stem over the rows primaries scaled by ``compensate``
            raws = [s.view(2, m.shape[1]) for m, s in zip(mixes, sec)]
            self.engine.demix_batch_dev([(m.data_ptr(), r.data_ptr(), m.shape[1]) for m, r in zip(mixes, raws)], is_match_mix=True,
                                        stream=self._stream())
            sec = [torch.empty((1024 * (m.shape[1] // 1024), 2), dtype=torch.float32, device=m.device) for m in mixes]
            self.engine.invert_stem_batch_dev([(r.data_ptr(), p.data_ptr(), m.shape[1], "rows", s.data_ptr(), s.shape[0])
                                               for m, r, p, s in zip(mixes, raws, prim, sec)], self.compensate, stream=self._stream())
        return list(zip(prim, sec))
