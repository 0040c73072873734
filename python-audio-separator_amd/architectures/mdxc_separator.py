"""MDXCSeparator on the HIP engine: drop-in for audio_separator/separator/architectures/mdxc_separator.py.

TFC-TDF v3 (MDX23C) checkpoints and BS / Mel-Band Roformer checkpoints; same constructor, ``load_model`` / ``separate`` /
``demix`` contract, stem dictionary, file naming and the "shorter than 10 s -> override_model_segment_size" rule
(:131-138).  ``torch.load`` + ``load_state_dict`` (:76-116) become ``asx_v3_*`` / ``asx_rof_*``; ``spec_utils.normalize`` of
the mix and of every stem (:147, :170-190) is ``asx_normalize``; the chunk loops are ``asx_mdxc_demix`` / ``asx_rof_demix``.
``separate_many(paths)`` (no counterpart in the reference) writes the files of ``separate`` per path with the chunks of all files
pooled per net pass (``asx_mdxc_demix_batch_dev`` / ``asx_rof_demix_batch_dev``).
"""
from __future__ import annotations


import numpy as np

from ..common_separator import CommonSeparator
from ..mdxc import MDXCDemixer


class MDXCSeparator(CommonSeparator):
    def __init__(self, common_config, arch_config):
        super().__init__(config=common_config)
        self._read_options(arch_config, (("segment_size", 256), ("override_model_segment_size", False), ("overlap", 8), ("batch_size", 1),
                                         ("pitch_shift", 0), ("process_all_stems", True)))
        # engine knob, not a reference option: most chunks one pooled call of separate_many takes (0 = what fits in HBM)
        self._pool_chunks = int(arch_config.get("asx_pool_chunks", 0))
        # ``separate_many(paths, custom_output_names=None)``: the shared batch shell, published on every instance rather than as a class
        # attribute (tests/test_host_vr_batch.py pins that the class itself carries no ``separate_many``)
        self.separate_many = self._separate_many
        self.logger.debug(f"MDXC arch params: batch_size={self.batch_size}, segment_size={self.segment_size}, overlap={self.overlap}, "
                          f"override_model_segment_size={self.override_model_segment_size}, pitch_shift={self.pitch_shift}")
        self.is_roformer = getattr(self, "is_roformer_model", False)
        if not self.is_roformer:                # TFC-TDF v3: convs and the fused TDF, no single-product kernels (common_separator.py: asx_autocast)
            if self.asx_autocast == "fp16":
                raise ValueError(f"asx_autocast='fp16' is not supported by {type(self).__name__} with a TFC-TDF v3 model: {self._AUTOCAST_ONLY_ROFORMER}")
            if self.asx_autocast == "follow":
                self.logger.info(f"asx_autocast='follow' does nothing for a TFC-TDF v3 model: {self._AUTOCAST_ONLY_ROFORMER}")
        self._keep_configs(common_config, arch_config)
        self._demixers = {}                 # one engine per chunk geometry (override_model_segment_size may flip per file)

        self.load_model()

        self._reset_file_state()
        training = self.model_data.get("training", {}) or {}
        self.is_primary_stem_main_target = bool(training.get("target_instrument"))
        self.logger.info(f"MDXC model ready ({'Roformer' if self.is_roformer else 'TFC-TDF v3'} on the HIP engine)")

    # ---- weights ---------------------------------------------------------------
    def _demixer(self, key=None) -> MDXCDemixer:
        """The demixer (and engine) of a chunk geometry: ``key`` True = the configured segment size, False = the model's own;
        None = the one ``override_model_segment_size`` selects now."""
        key = bool(self.override_model_segment_size if key is None else key)
        dm = self._demixers.get(key)
        if dm is None:
            common = dict(self._common)
            common["logger"] = self.logger
            common["primary_stem_name"], common["secondary_stem_name"] = self.primary_stem_name, self.secondary_stem_name
            arch = dict(self._arch)
            arch["override_model_segment_size"] = key
            dm = MDXCDemixer(common, arch, state_dict=self._state_dict, max_batch=self._max_batch)
            if self.roformer_loader is not None and getattr(dm, "roformer_loader", None) is not None:
                self.roformer_loader._loading_stats = dm.roformer_loader.get_loading_stats()
            self._demixers[key] = dm
        dm.overlap = self.overlap
        self.engine = dm.engine
        return dm

    def load_model(self):
        """mdxc_separator.py:76-116: the checkpoint is read once; a failing / corrupt file exits like the reference."""
        import sys
        from ..model_files import read_state_dict
        from ..roformer_config import read_checkpoint
        self._state_dict = self._common.get("asx_state_dict")
        try:
            if self._state_dict is None:
                self._state_dict = read_checkpoint(self.model_path) if self.is_roformer else read_state_dict(self.model_path)
            self._demixer()
        except RuntimeError as e:
            # same outcome as the reference (mdxc_separator.py:108-116): a checkpoint that cannot be read ends the process
            self.logger.error(f"{self.model_path}: the checkpoint could not be loaded ({e}); the file is probably truncated or "
                              "corrupt -- delete it so that it is fetched again")
            sys.exit(1)

    # ---- the path ----------------------------------------------------------------
    def demix(self, mix: np.ndarray):
        """mdxc_separator.py:257-468: dict of stems, or the primary array for a single-target model without residual."""
        return self._demixer().demix(mix)

    def _short_file_rule(self, seconds):
        """mdxc_separator.py:131-138."""
        if seconds < 10.0 and not self.override_model_segment_size:
            self.override_model_segment_size = True
            self.logger.warning(f"{seconds:.2f} s of audio (< 10 s): switching to the configured segment size "
                                "(override_model_segment_size), as the reference does for short files")

    def _complement_stem_name(self):
        """The residual row of a single-target model, ``mix - primary`` (also with ``pitch_shift``: it is taken against the original mix);
        a model without ``target_instrument`` has none."""
        training = self.model_data.get("training", {}) or {}
        return self.secondary_stem_name if training.get("target_instrument") else None

    def _stem_plan(self, names):
        """What ``separate`` writes of a demix that produced the stems ``names`` (``[None]``: the one array of a single-target
        model without residual): (kind, [(stem name, key into the demix)]) in the order written.  "single": the primary stem;
        "all": every stem of a multi-stem model, ``output_single_stem`` does not apply; "pair": secondary first."""
        if names == [None]:
            return "single", [(self.primary_stem_name, None)]
        training = self.model_data.get("training", {}) or {}
        order = [training["target_instrument"]] if training.get("target_instrument") else list(training.get("instruments") or [])
        if self.process_all_stems and len(order) > 2:
            return "all", [(k, k) for k in order]
        return "pair", [(k, k) for k in (self.secondary_stem_name, self.primary_stem_name)]

    def _device_stems(self):
        """The stems of the current file with every array in HBM (RIFF/WAVE input at the model's rate): decode on the device,
        normalise the mix in place (asx_normalize_dev), demix, residual stem, normalise every stem in place.  Returns
        (stems [S, 2, N] CUDA tensor, kind, [(stem name, row of ``stems``)]) as ``_stem_plan`` has them.  None: take the
        generic path.  With ``pitch_shift`` the round trip runs inside ``demix_dev`` (mdxc.py ``_pitched_many_dev``)."""
        if self.engine is None:
            self._demixer()
        mix_d = self._device_mix(self.audio_file_path)
        if mix_d is None:
            return None
        n = mix_d.shape[1]
        self._short_file_rule(n / self.sample_rate)
        dm = self._demixer()
        if dm.engine.device != mix_d.device.index:
            return None
        t0 = self._now()
        eng, st = dm.engine, self._stream()
        thr, amp = self.normalization_threshold, self.amplification_threshold
        self._mix_scale = self._mix_factor(mix_d, None)
        eng.normalize_dev(mix_d.data_ptr(), 2 * n, thr, amp, stream=st)
        names, stems_d = dm.demix_dev(mix_d)
        self.last_arithmetic = dm.last_arithmetic
        kind, entries = self._stem_plan(names)
        entries = [(name, names.index(key)) for name, key in entries]
        if kind != "single":
            for i in sorted({i for _, i in entries}):     # norm(source[name]) of the reference, once per stem, in place
                eng.normalize_dev(stems_d[i].data_ptr(), 2 * n, thr, amp, stream=st)
        self._tick("demix", t0)
        return stems_d, kind, entries

    def stems_dev(self, audio_file_path):
        """The stems ``separate(audio_file_path)`` would hand to write_audio, in its order, left on the device:
        [(stem name, CUDA tensor [2, N], "planar")]; honours ``output_single_stem`` where ``separate`` does and carries the
        residual stem of a single-target model.  None when the file needs the host decoder.  Writes nothing."""
        self._reset_file_state()
        self._begin_file(audio_file_path)
        self._stems_only = True                           # (nothing is written: asx_complement_rate has no use for the file's mix)
        try:
            got = self._device_stems()
        finally:
            self._stems_only = False
        return None if got is None else self._stems_of(got)

    def _stems_of(self, got):
        """(stems [S, 2, N], kind, entries) as ``_device_stems`` and ``_pooled_stems`` have them -> the list ``stems_dev`` returns."""
        if isinstance(got, Exception):
            raise got
        if got[0] == "host":                              # no device file path: host stems
            return None
        stems_d, kind, entries = got
        return [(name, stems_d[i], "planar") for name, i in entries if kind == "all" or self._wanted(name)]

    stems_dev_many = CommonSeparator._stems_dev_many

    def _emit_plan(self, kind, entries, fetch, custom_output_names):
        """``_stem_plan`` -> files; ``fetch(key)`` is the [N, 2] array of one stem, called once per stem.  ``separate`` has reset
        the file state, so ``primary_source`` / ``secondary_source`` are always this file's."""
        files = []
        if kind != "pair" or self._complement_stem_name() is None:
            self._note_no_complement(f"no stem of {self.model_name} is a residual against the mix")
            self._file_mix = None
        if kind == "all":
            for name, key in entries:
                self._emit_stem(name, fetch(key), custom_output_names, files)
        elif kind == "pair":
            self.primary_source, self.secondary_source = fetch(entries[1][1]), fetch(entries[0][1])
            if self._complement_stem_name() is not None:
                # asx_complement_rate = "input": the residual's file is written from s * (the file's mix) - (the converted primary), then
                # normalised like every stem of this plugin
                self._register_complement(self.secondary_source, self.primary_source, 1.0, True,
                                          model_wanted=self._wanted(self.primary_stem_name))
            files = self._emit_pair(custom_output_names)
        elif self._wanted(self.primary_stem_name):        # "single" (mdxc_separator.py:213-225)
            self.primary_source = fetch(entries[0][1])
            self.primary_stem_output_path = self._emit_stem(self.primary_stem_name, self.primary_source, custom_output_names, files)
        return files

    def separate(self, audio_file_path, custom_output_names=None):
        """mdxc_separator.py:118-227."""
        self._reset_file_state()
        self._begin_file(audio_file_path)
        got = self._device_stems()
        if got is not None:
            # host mirrors (pinned) of the device stems as the sources; the int16 pass of each written stem runs on the device
            stems_d, kind, entries = got
            t0 = self._now()
            _, views = self._host_planar_stems(stems_d)
            self._sync()
            self._tick("stems_d2h", t0)
            return self._emit_plan(kind, entries, views.__getitem__, custom_output_names)
        mix = self.prepare_mix(self.audio_file_path)
        self._short_file_rule(mix.shape[1] / self.sample_rate)
        dm = self._demixer()
        self._mix_scale = self._mix_factor(None, mix)
        norm = lambda w: dm.engine.normalize(w, self.normalization_threshold, self.amplification_threshold)   # noqa: E731
        source = dm.demix(norm(np.ascontiguousarray(mix, np.float32)))
        self.last_arithmetic = dm.last_arithmetic
        kind, entries = self._stem_plan(list(source) if isinstance(source, dict) else [None])
        # (the one array of a "single" plan goes to the writer as it is; every other stem is normalised when it is fetched)
        return self._emit_plan(kind, entries, lambda key: source.T if key is None else norm(source[key]).T, custom_output_names)

    # ---- a batch of files: the hooks of CommonSeparator._separate_many ------------------------------------------------------
    # A loop of ``separate`` switches ``override_model_segment_size`` on at the first file under 10 s and leaves it on, so the files
    # before that one run the model's chunk geometry and that file and all later ones the configured one: at most two pools, each on
    # its own engine.  ``_check_loaded`` applies the rule in file order and records every good file's geometry.
    def _prepare_model(self):
        self._pool_keys = []
        if self.engine is None:
            self._demixer()

    def _check_loaded(self, dev_mix, host_mix):
        """The short-file rule, then what ``demix`` would refuse: such a file fails alone and never reaches the pooled call, which
        rejects a whole pool for one Roformer mix shorter than a chunk."""
        mix = dev_mix if dev_mix is not None else host_mix
        n = mix.shape[1]
        self._short_file_rule(n / self.sample_rate)
        key = bool(self.override_model_segment_size)
        if mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got {mix.shape[0]} channels")
        if self.is_roformer and (self.pitch_shift == 0 or self._fast_file_path_enabled()):
            # with pitch_shift the net sees the pitched mix.  Every file of the batch, host-decoded ones too, reaches the pooled device call
            # when the device file path is on, and that call refuses a whole pool for one short mix; without the device file path the batch
            # is the loop of demix, which refuses such a file itself, alone, as before
            dm = self._demixer(key)
            seen, what = (n, "mix") if self.pitch_shift == 0 else (dm.pitched_len(n), "pitched mix")
            if seen < dm.chunk_size:
                raise ValueError(f"{what} ({seen} samples) shorter than one chunk ({dm.chunk_size}): not supported on the Roformer path")
        self._pool_keys.append(key)

    def _sub_pools(self, dm, lengths):
        """Consecutive runs of files, in order, whose chunks fit one pooled call: the pooled chunk buffer ([chunks, S, 2, chunk]
        floats) stays within 60 % of the HBM that is free now, or within ``asx_pool_chunks`` chunks when that is set.  A file that
        alone exceeds the budget is a run of its own (the single-song call would need the same buffer).  With ``pitch_shift`` the net
        sees the pitched mixes: the chunks are counted from their lengths, and the temporaries of the round trip -- the pitched mix
        [2, n'] and the stems at the pitched rate [rows, 2, n'] of every song of a run -- count against the HBM budget, in chunks
        (``asx_pool_chunks`` counts chunks alone; the result rows [rows + 1, 2, N] are the caller's and are not charged, with or without
        the option).  tests/test_gpu_mdxc_pitch_dev.py holds the charge against the allocator's peak beside the results.  The file-rate
        mixes that ``asx_complement_rate`` = "input" keeps per song (8 bytes a frame) are resident when the free HBM is read here, so the
        HBM budget is already net of them; ``asx_pool_chunks`` counts chunks alone and so counts neither them nor the pitch temporaries."""
        extra = [0] * len(lengths)
        if self.pitch_shift != 0:
            lengths = [dm.pitched_len(n) for n in lengths]
        if dm.is_roformer:
            step, rows = dm.roformer_step(), int(dm.rof.num_stems)
            counts = [-(-n // step) for n in lengths]
        else:
            rows = int(dm.v3.num_targets)
            hop = dm.chunk_size // int(dm.overlap)
            counts = [(n + hop - (n - dm.chunk_size) % hop + dm.chunk_size - hop) // hop for n in lengths]    # Tensor.unfold's count
        budget = self._pool_chunks
        if budget <= 0:
            budget = 1 << 30
            try:
                import torch
                free, _total = torch.cuda.mem_get_info(dm.engine.device)
                budget = max(1, int(0.6 * free / (rows * 2 * dm.chunk_size * 4)))
                if self.pitch_shift != 0:
                    out_rows = max(rows, int(dm.rof.n_out)) if dm.is_roformer else rows
                    extra = [-(-(out_rows + 1) * n // (rows * dm.chunk_size)) for n in lengths]
            except Exception:      # no device query: one pool, the engine reports an allocation failure itself
                pass
        runs, used = [[]], 0
        for i, c in enumerate(c + x for c, x in zip(counts, extra)):
            if runs[-1] and used + c > budget:
                runs.append([])
                used = 0
            runs[-1].append(i)
            used += c
        return runs

    def _pooled_stems(self, mixes):
        """Per file what ``_emit_file`` takes.  Files on the device path: normalise each mix in place, ONE pooled demix per geometry
        (``MDXCDemixer.demix_many_dev``; split into consecutive sub-pools only for memory), normalise every stem in place -- exactly
        where ``_device_stems`` does.  Without the device file path (``ASX_FILE_FASTPATH=0``) the same pools run through
        ``demix_many`` on host arrays -- with ``pitch_shift`` the loop of ``demix`` per file (mdxc.py ``demix_many``); on the device path
        the pitch round trip is part of ``demix_many_dev``."""
        keys, self._pool_keys = self._pool_keys, []
        thr, amp = self.normalization_threshold, self.amplification_threshold
        out = [None] * len(mixes)
        kept = getattr(self, "_pool_kept", None) or [False] * len(mixes)
        scales = self._pool_mix_scales = [1.0] * len(mixes)       # the factor of each mix's normalise, read before it runs
        host_only = not self._fast_file_path_enabled()
        for key in (False, True):
            idx = [i for i, k in enumerate(keys) if k == key]
            if not idx:
                continue
            dm = self._demixer(key)
            eng = dm.engine
            dm._set_arithmetic()                         # one arithmetic per pooled call (every demix below sets the same again)
            self._pool_arithmetic = dm.last_arithmetic   # -> every file's per-file state (CommonSeparator._pool_files)
            if host_only and self.pitch_shift != 0:
                for i in idx:
                    try:
                        scales[i] = self._mix_factor(None, mixes[i][1], kept[i])
                        out[i] = ("host", eng, dm.demix(eng.normalize(mixes[i][1], thr, amp)))
                    except Exception as e:                   # this file only: raised again where its files would be written
                        out[i] = e
                continue
            if host_only:
                host = [mixes[i][1] if mixes[i][1] is not None else mixes[i][0].cpu().numpy() for i in idx]
                for i, m in zip(idx, host):
                    scales[i] = self._mix_factor(None, m, kept[i])
                host = [eng.normalize(m, thr, amp) for m in host]
                for run in self._sub_pools(dm, [m.shape[1] for m in host]):
                    for j, source in zip(run, dm.demix_many([host[j] for j in run])):
                        out[idx[j]] = ("host", eng, source)
                continue
            t0 = self._now()
            st = self._stream()
            dev = self._device_mixes([mixes[i] for i in idx])
            for i, m in zip(idx, dev):
                scales[i] = self._mix_factor(m, None, kept[i])
                eng.normalize_dev(m.data_ptr(), 2 * m.shape[1], thr, amp, stream=st)
            for run in self._sub_pools(dm, [m.shape[1] for m in dev]):
                for j, (names, stems_d) in zip(run, dm.demix_many_dev([dev[j] for j in run])):
                    kind, entries = self._stem_plan(names)
                    entries = [(name, names.index(k)) for name, k in entries]
                    if kind != "single":
                        for r in sorted({r for _, r in entries}):
                            eng.normalize_dev(stems_d[r].data_ptr(), 2 * stems_d.shape[2], thr, amp, stream=st)
                    out[idx[j]] = (stems_d, kind, entries)
            self._tick("demix", t0)
        return out

    def _emit_file(self, stems, on_device, custom_output_names):
        """One entry of ``_pooled_stems`` -> the file's outputs, as ``separate`` ends.  Device stems of a file decoded on the device
        keep their device tensors for the int16 pass; a host-decoded file's stems take the host writer."""
        if isinstance(stems, Exception):
            raise stems
        if stems[0] == "host":
            _, eng, source = stems
            norm = lambda w: eng.normalize(w, self.normalization_threshold, self.amplification_threshold)   # noqa: E731
            kind, entries = self._stem_plan(list(source) if isinstance(source, dict) else [None])
            return self._emit_plan(kind, entries, lambda k: source.T if k is None else norm(source[k]).T, custom_output_names)
        stems_d, kind, entries = stems
        if on_device:
            t0 = self._now()
            _, views = self._host_planar_stems(stems_d)
            self._sync()
            self._tick("stems_d2h", t0)
            return self._emit_plan(kind, entries, views.__getitem__, custom_output_names)
        host = self._to_host(stems_d)
        return self._emit_plan(kind, entries, lambda r: host[r].T, custom_output_names)
