"""Multi-model ensembles with resident members: ``Separator._separate_ensemble`` (audio_separator/separator/separator.py:1242-1392)
and ``Ensembler`` (audio_separator/separator/ensembler.py) on the HIP engine.

The reference runs K models on one song by reloading each model, writing every stem of every model to a temporary
directory as a 16-bit file, reading the files back with librosa and combining equal-named stems in numpy.
``EnsembleSeparator`` keeps the K plugin instances (and their engines) loaded and offers two paths in one class:

* ``via_files=True`` -- that literal flow, minus the reloads: ``member.separate`` into a temporary directory, the files read
  back (audio_io), ``Engine.ensemble`` on the host arrays, ``write_audio``.  Every piece of it is pinned to reference goldens.
* the default -- the same result without a file or a host float array between the members and the combine: each member's
  ``stems_dev`` leaves its stems in HBM, ``asx_ensemble_slot_dev`` applies what the file round trip does to the samples
  (spec_utils.normalize, ``* 32767 -> int16``, ``/ 32768``, zero padding to the longest contributor) while filling the stack
  ``asx_ensemble_dev`` reads, and the result is registered as a device stem so that ``write_audio`` quantises it there.
  Outputs are byte-identical to the file path.  ``intermediate="writer"`` gives every contributor the round trip of its own
  member's writer (the soundfile writer's PCM_16 / PCM_24 / PCM_32 / FLOAT files included), so members with ``use_soundfile`` stay
  on this path; ``output_rate="input"`` has the last member's writer convert the combined result to the input file's rate.

``Ensembler`` is the drop-in for the reference class of that name (``plugin.install(ensembler=True)``).
"""
from __future__ import annotations

import logging
import os
import re
import shutil
import tempfile

import numpy as np

from . import audio_io

# separator.py:29-49, restated: lower-cased stem label -> the group it is ensembled in
STEM_NAME_MAP = {
    "vocals": "Vocals", "instrumental": "Instrumental", "inst": "Instrumental", "karaoke": "Instrumental", "other": "Other",
    "no_vocals": "Instrumental", "drums": "Drums", "bass": "Bass", "guitar": "Guitar", "piano": "Piano",
    "synthesizer": "Synthesizer", "strings": "Strings", "woodwinds": "Woodwinds", "brass": "Brass", "wind inst": "Wind Inst",
    "lead vocals": "Lead Vocals", "backing vocals": "Backing Vocals", "primary stem": "Primary Stem",
    "secondary stem": "Secondary Stem",
}
# separator.py:1362: prefixes dropped from a model file name before it is cut to 12 characters (the first match only)
_SLUG_PREFIXES = ("mel_band_roformer_", "melband_roformer_", "bs_roformer_", "model_bs_roformer_", "UVR-MDX-NET-", "UVR_MDXNET_")
_SILENT = 1e-6          # write_audio writes no file for a stem whose peak after normalisation is below this
_LOSSLESS_16 = ("wav", "flac")


def raw_stem_name(stem_file_name: str) -> str:
    """separator.py:1291-1293: the stem label is whatever the FIRST ``_(...)`` of the intermediate file's basename holds -- for an
    input called ``song_(live).wav`` that is ``live`` for every stem; kept, the files the reference writes depend on it."""
    match = re.search(r"_\(([^)]+)\)", os.path.basename(stem_file_name))
    return match.group(1) if match else "Unknown"


def canonical_stem_names(raw_names) -> list:
    """separator.py:1296-1315 for the stems ONE model produced: the group name of each."""
    has_vocal_stem = any("vocal" in s.lower() for s in raw_names)
    out = []
    for raw in raw_names:
        lower = raw.lower()
        if "vocal" in lower and "lead" not in lower and "backing" not in lower:
            out.append("Vocals")
        elif lower == "other" and len(raw_names) == 2 and has_vocal_stem:
            out.append("Instrumental")            # the complement of the vocals in a 2-stem model
        elif lower in STEM_NAME_MAP:
            out.append(STEM_NAME_MAP[lower])
        else:
            out.append(raw.title())
    return out


def model_slugs(model_filenames) -> str:
    """separator.py:1357-1367."""
    slugs = []
    for mf in model_filenames:
        name = os.path.splitext(mf)[0]
        for prefix in _SLUG_PREFIXES:
            if name.startswith(prefix):
                name = name[len(prefix):]
                break
        slugs.append(name[:12])
    return "_".join(slugs)


def ensemble_output_name(base_name, stem_name, custom_output_names=None, preset=None, model_filenames=()) -> str:
    """separator.py:1350-1368 (without the extension)."""
    if custom_output_names and stem_name in custom_output_names:
        return custom_output_names[stem_name]
    if preset:
        return f"{base_name}_({stem_name})_preset_{preset}"
    return f"{base_name}_({stem_name})_custom_ensemble_{model_slugs(model_filenames)}"


def effective_weights(weights, k: int, logger=None):
    """ensembler.py:32-44: the weights a combine of ``k`` waves really uses, as float64 -- ones for None, a length mismatch,
    a non-finite value or a zero sum."""
    if weights is None:
        return np.ones(k)
    w = np.array(weights, dtype=np.float64)
    if len(w) != k:
        if logger:
            logger.warning(f"Number of weights ({len(w)}) does not match number of waveforms ({k}). Using equal weights.")
        return np.ones(k)
    total = np.sum(w)
    if not np.all(np.isfinite(w)) or not np.isfinite(total) or total == 0:
        if logger:
            logger.warning(f"Weights {weights} contain non-finite values or sum to zero. Falling back to equal weights.")
        return np.ones(k)
    return w


def file_rate_of(member, path):
    """(sample rate, frames) of the file ``member`` has just loaded -- what its decoder recorded, or the file's own header where it
    recorded nothing; (None, None) when neither is known (a writer handed that as its ``_output_rate_override`` warns once and writes
    at the model's rate)."""
    rate, frames = getattr(member, "_file_rate", None), getattr(member, "_file_frames", None)
    if rate and frames:
        return rate, frames
    try:
        info = audio_io.wav_info(path)
        return info["samplerate"], info["frames"]
    except Exception:
        try:
            info = audio_io.flac_stream(path)
            return (info["samplerate"], info["total_samples"]) if info["total_samples"] > 0 else (None, None)
        except Exception:
            return None, None


def stems_per_file(member):
    """Stems ``member`` keeps per file, for the memory estimate of a pooled run (an upper bound where the model decides)."""
    if hasattr(member, "demucs_source_map") or hasattr(member, "demucs_model_instance"):
        return 6
    instruments = ((getattr(member, "model_data", None) or {}).get("training") or {}).get("instruments") or []
    return len(instruments) if getattr(member, "process_all_stems", False) and len(instruments) > 2 else 2


def free_hbm(device):
    try:
        import torch
        return torch.cuda.mem_get_info(device)[0]
    except Exception:        # no device query: one run, an allocation failure is reported where it happens
        return None


def pooled_runs(paths, pool_files, free, per_frame, share):
    """``paths`` as consecutive runs of indices, in order -- the files one pooled call of resident members serves (EnsembleSeparator,
    PhaseFixSeparator).  ``pool_files`` set: that many per run.  Else a run's estimated stem bytes -- frames (audio_io.wav_info, or a
    FLAC stream's total_samples) x ``per_frame`` bytes -- stay within ``share`` of the free HBM (``free()``; None: one run); a run of
    one file is always allowed."""
    if not paths:
        return []
    if pool_files is not None:
        return [list(range(i, min(i + pool_files, len(paths)))) for i in range(0, len(paths), pool_files)]
    free = free()
    if free is None:
        return [list(range(len(paths)))]
    runs, used = [[]], 0
    for i, path in enumerate(paths):
        try:
            cost = audio_io.wav_info(path)["frames"] * per_frame
        except Exception:    # not a RIFF/WAVE file: a FLAC stream by STREAMINFO's sample count where it gives one; anything else takes the
            try:             # file path or fails, no stems are kept for it
                cost = audio_io.flac_stream(path)["total_samples"] * per_frame
            except Exception:
                cost = 0
        if runs[-1] and used + cost > share * free:
            runs.append([])
            used = 0
        runs[-1].append(i)
        used += cost
    return runs


class EnsembleSeparator:
    ALGORITHMS = ("avg_wave", "median_wave", "min_wave", "max_wave", "avg_fft", "median_fft", "min_fft", "max_fft",
                  "uvr_max_spec", "uvr_min_spec", "ensemble_wav")

    INTERMEDIATES = ("pcm16", "float32", "writer")
    OUTPUT_RATES = ("model", "input")
    # the sample formats a soundfile member's intermediate file can carry on the device path (Engine.SLOT_MODES, asx_pcm_encode_dev)
    _WRITER_SUBTYPES = ("PCM_16", "PCM_24", "PCM_32", "FLOAT")

    def __init__(self, members, algorithm="avg_wave", weights=None, preset=None, model_filenames=None, intermediate="pcm16",
                 via_files=False, logger=None, pool_files=None, output_rate="model"):
        """``members``: loaded plugin instances (MDXSeparator / MDXCSeparator / DemucsSeparator / VRSeparator, any mix); they
        and their engines stay resident across files.  ``algorithm`` / ``weights``: Ensembler's.  ``preset`` only names the
        outputs (``..._preset_<preset>``); ``model_filenames`` (default: each member's model file basename) name them
        otherwise.  ``intermediate``: "pcm16" (what the reference's 16-bit intermediate files carry, the default),
        "float32" (unquantised stems between members and combine; device path only) or "writer" (every contributor's stem takes
        the round trip its OWN member's writer and audio_io.load give it for this file: pcm16 for a member without
        ``use_soundfile``, the file's own PCM_16 / PCM_24 / PCM_32 / FLOAT for one with it -- so soundfile members stay on the
        device path).  ``via_files``: the literal flow.  ``pool_files``: files per pooled run of ``separate_many`` (None: as many
        as the memory rule allows).  ``output_rate``: "model" (the default) or "input": the combined result -- and only it; members,
        intermediates and the combine stay at the model's rate -- is written at the input file's sample rate and frame count,
        converted inside the last member's ``write_audio`` as ``asx_output_rate`` = "input" converts a single plugin's stems."""
        self.members = list(members)
        if not self.members:
            raise ValueError("an ensemble needs at least one member")
        if algorithm not in self.ALGORITHMS:
            raise ValueError(f"Unknown ensemble algorithm: {algorithm}")
        if intermediate not in self.INTERMEDIATES:
            raise ValueError(f"intermediate must be 'pcm16', 'float32' or 'writer', not {intermediate!r}")
        if output_rate not in self.OUTPUT_RATES:
            raise ValueError(f"output_rate must be one of {self.OUTPUT_RATES}, not {output_rate!r}")
        if output_rate == "input":
            for m in self.members:
                if getattr(m, "_output_rate_refusal", None):
                    # the knob's own refusal (CommonSeparator._output_rate_mode): a member that cannot line up with the file at its rate
                    raise ValueError(f"output_rate='input' is not supported with a {type(m).__name__} member: {m._output_rate_refusal}")
        if intermediate == "float32" and via_files:   # ("writer" with via_files is the literal flow itself)
            raise ValueError("intermediate='float32' is an option of the device path (via_files=False): the file path's "
                             "intermediates are the 16-bit files")
        first = self.members[0]
        for key in ("sample_rate", "normalization_threshold", "amplification_threshold"):
            values = [getattr(m, key) for m in self.members]
            if any(v != values[0] for v in values):
                # the orchestrator hands every model the same values; intermediates are not resampled between rates
                raise ValueError(f"ensemble members differ in {key}: {values}")
        modes = [getattr(m, "asx_input_resample", "host") for m in self.members]
        if any(v != modes[0] for v in modes):
            # a file at another rate would reach the members through different converters (or fail in some of them only)
            raise ValueError(f"ensemble members differ in asx_input_resample: {modes}")
        if any(getattr(m, "asx_output_rate", "model") == "input" for m in self.members):
            # the intermediates and the combine live at the model's rate: a member at "input" would hand the file path stems at another
            raise ValueError("asx_output_rate='input' is not supported in an ensemble: the intermediates and the combine stay at the "
                             "model's rate; leave the members at 'model' and pass output_rate='input' to EnsembleSeparator, which "
                             "converts the combined result")
        if model_filenames is not None and len(model_filenames) != len(self.members):
            raise ValueError(f"{len(model_filenames)} model file names for {len(self.members)} members")
        self.algorithm, self.weights, self.preset = algorithm, weights, preset
        self.intermediate, self.via_files, self.output_rate = intermediate, bool(via_files), output_rate
        self.model_filenames = list(model_filenames) if model_filenames is not None else [
            os.path.basename(m.model_path) if m.model_path else str(m.model_name) for m in self.members]
        self.logger = logger or first.logger or logging.getLogger("audio_separator_amd")
        self.sample_rate = first.sample_rate
        writer = self.members[-1]                   # separator.py:1372-1379: the model loaded last writes the result
        self.output_dir, self.output_format = writer.output_dir, writer.output_format
        if pool_files is not None and int(pool_files) < 1:
            raise ValueError(f"pool_files must be at least 1, not {pool_files!r}")
        self.pool_files = None if pool_files is None else int(pool_files)
        self.last_path_taken = None                 # "device" | "files": the path the last input took
        self.last_paths_taken = []                  # separate_many: "device" | "files" | "failed" per input
        self.batch_errors = {}                      # separate_many: input index -> the exception that file raised

    # ---- shared pieces ---------------------------------------------------------------------------------------------
    def _group_names(self, member, stem_names):
        """The ensemble group of each stem ``member`` produced for the current file, from the file names it gives them."""
        return canonical_stem_names([raw_stem_name(member.get_stem_output_path(n, None)) for n in stem_names])

    def _write(self, path, stem_name, source, custom_output_names, file_rate=None):
        """separator.py:1350-1381: name the result, let the last member write it; ``source`` is [N, 2].  ``file_rate``: what
        ``_file_rate_of`` returned for this file -- under ``output_rate`` = "input" the writer converts the result to it, for this
        call only (``CommonSeparator._output_rate_override``); its own ``asx_output_rate`` is not touched."""
        writer = self.members[-1]
        base_name = os.path.splitext(os.path.basename(path))[0]
        name = ensemble_output_name(base_name, stem_name, custom_output_names, self.preset, self.model_filenames)
        output_path = f"{name}.{self.output_format.lower()}"
        writer.audio_file_path = path
        writer.output_dir = self.output_dir
        writer._output_rate_override = file_rate
        try:
            writer.write_audio(output_path, source)
        finally:
            writer._output_rate_override = None
        return os.path.join(self.output_dir, output_path) if self.output_dir else output_path

    def _file_rate_of(self, member, path):
        """Under ``output_rate`` = "input": ``file_rate_of(member, path)``.  None under "model": no override."""
        return file_rate_of(member, path) if self.output_rate == "input" else None

    def _slot_mode(self, member):
        """(slot mode, None) of the stems ``member`` produced for the file it has just loaded -- ``Engine.SLOT_MODES``' name of the round
        trip its writer plus audio_io.load would give them -- or (None, why) when only its real intermediate file tells."""
        if self.intermediate != "writer":
            return self.intermediate, None
        if not member.use_soundfile:
            return "pcm16", None                    # write_audio_pydub: the reference's 16-bit samples
        subtype = member._output_subtype()
        fmt = str(member.output_format).lower()
        if subtype not in self._WRITER_SUBTYPES:
            return None, f"writes {subtype} intermediates, which have no device round trip"
        if fmt == "flac" and subtype in ("PCM_32", "FLOAT"):
            return None, f"writes no intermediate at all: FLAC holds no {subtype} samples"
        if not member._soundfile_on_device(f"stem.{fmt}"):
            return None, "writes its intermediates with soundfile on the host"
        return subtype, None

    def _device_path_refusal(self):
        """Why an input cannot take the device path, or None."""
        if self.via_files:
            return "via_files=True"
        if self.intermediate != "writer" and any(m.use_soundfile for m in self.members):
            return "a member writes with soundfile (float intermediates, not the 16-bit round trip)"
        if str(self.output_format).lower() not in _LOSSLESS_16:
            return f"output_format {self.output_format} is not one of {_LOSSLESS_16} (the intermediates would not be lossless 16-bit)"
        if any(not hasattr(m, "stems_dev") for m in self.members):
            return "a member has no device-stem hook"
        return None

    # ---- the public call ---------------------------------------------------------------------------------------------
    def separate(self, audio_file_path, custom_output_names=None):
        """``Separator._separate_ensemble``: a path or a list of paths -> the output files of all of them, in order."""
        paths = [audio_file_path] if isinstance(audio_file_path, str) else list(audio_file_path)
        output_files = []
        for path in paths:
            self.logger.info(f"Ensemble processing for file: {path}")
            files = None
            why = self._device_path_refusal()
            if why is None:
                files = self._separate_on_device(path, custom_output_names)
            elif not self.via_files:
                self.logger.info(f"{path}: ensemble through intermediate files ({why})")
            if files is None:
                files = self._separate_via_files(path, custom_output_names)
                self.last_path_taken = "files"
            else:
                self.last_path_taken = "device"
            output_files.extend(files)
        return output_files

    # ---- the literal flow ----------------------------------------------------------------------------------------------
    def _separate_via_files(self, path, custom_output_names):
        temp_dir = tempfile.mkdtemp(prefix="audio-separator-ensemble-")
        try:
            stems_by_type = {}
            for member in self.members:
                saved = member.output_dir
                member.output_dir = temp_dir
                try:
                    # no custom names for the intermediates: their default names carry the stem labels (separator.py:1282-1286)
                    model_stems = member.separate(path, None)
                    file_rate = self._file_rate_of(member, path)          # (the last member's is the writer's)
                    member.clear_gpu_cache()
                    member.clear_file_specific_paths()
                finally:
                    member.output_dir = saved
                groups = canonical_stem_names([raw_stem_name(p) for p in model_stems])
                for stem_path, group in zip(model_stems, groups):
                    full = stem_path if os.path.isabs(stem_path) else os.path.join(temp_dir, stem_path)
                    stems_by_type.setdefault(group, []).append(full)
            engine = self.members[-1].engine
            outputs = []
            for stem_name, stem_paths in stems_by_type.items():
                waveforms, original_channels = [], None
                for sp in stem_paths:
                    if not os.path.isfile(sp):
                        # the member's writer left a silent stem out (peak < 1e-6); the reference would fail on loading it
                        self.logger.warning(f"{stem_name}: {os.path.basename(sp)} was not written (silent stem), left out of the ensemble")
                        continue
                    wav, _ = audio_io.load(sp, mono=False, sr=self.sample_rate)
                    if wav.ndim == 1:
                        if original_channels is None:
                            original_channels = 1
                        wav = np.asfortranarray([wav, wav])
                    elif original_channels is None:
                        original_channels = wav.shape[0]
                    waveforms.append(wav)
                if not waveforms:
                    continue
                self.logger.info(f"Ensembling {len(waveforms)} stems for type: {stem_name}")
                ensembled = engine.ensemble(waveforms, self.algorithm, self.weights)
                if original_channels == 1 and ensembled.shape[0] > 1:
                    ensembled = ensembled[:1, :]
                outputs.append(self._write(path, stem_name, ensembled.T, custom_output_names, file_rate))
            return outputs
        finally:
            shutil.rmtree(temp_dir, ignore_errors=True)

    # ---- the same without files ----------------------------------------------------------------------------------------
    def _separate_on_device(self, path, custom_output_names):
        """None: this input needs the file path (a member could not keep its stems on the device)."""
        import torch
        writer = self.members[-1]
        groups = {}                                  # group name -> [(member index, device stem, layout)], first-seen order
        for index, member in enumerate(self.members):
            stems = member.stems_dev(path)
            if stems is None:
                self.logger.info(f"{path}: ensemble through intermediate files (member {index}, {member.model_name}, needs the host decoder)")
                member.clear_file_specific_paths()
                return None
            names = self._group_names(member, [name for name, _, _ in stems])
            mode, why = self._slot_mode(member)
            file_rate = self._file_rate_of(member, path)                  # (the last member's is the writer's)
            member.clear_file_specific_paths()
            if mode is None:
                self.logger.info(f"{path}: ensemble through intermediate files (member {index}, {member.model_name}, {why})")
                return None
            for (_, tensor, layout), group in zip(stems, names):
                groups.setdefault(group, []).append((index, tensor, layout, mode))
        engine = writer.engine
        if any(t.device.index != engine.device for contributors in groups.values() for _, t, _, _ in contributors):
            self.logger.info(f"{path}: ensemble through intermediate files (members sit on different devices)")
            return None
        thr, amp = writer.normalization_threshold, writer.amplification_threshold
        stream = writer._stream()
        outputs = []
        for stem_name, contributors in groups.items():
            live = list(contributors)
            stack = None
            while live:
                # Ensembler.ensemble pads to the longest wave it is GIVEN: a silent stem (no file in the reference) counts for neither
                n_max = max(t.shape[1] if layout == "planar" else t.shape[0] for _, t, layout, _ in live)
                stack = torch.empty((len(live), 2, n_max), dtype=torch.float32, device=live[0][1].device)
                peaks = []
                for k, (_, t, layout, mode) in enumerate(live):
                    if not t.is_contiguous():
                        t = t.contiguous()
                    n = t.shape[1] if layout == "planar" else t.shape[0]
                    peaks.append(engine.ensemble_slot_dev(t.data_ptr(), n, layout, thr, amp, stack.data_ptr(), k, n_max,
                                                          mode=mode, stream=stream))
                silent = [c for c, p in zip(live, peaks) if p < _SILENT]
                if not silent:
                    break
                for index, _, _, _ in silent:
                    self.logger.warning(f"{stem_name}: the stem of member {index} ({self.members[index].model_name}) is silent, left out of the ensemble")
                live = [c for c, p in zip(live, peaks) if not p < _SILENT]
            if not live:
                continue
            self.logger.info(f"Ensembling {len(live)} stems for type: {stem_name}")
            k, n_max = stack.shape[0], stack.shape[2]
            if k == 1:
                result = stack                       # a lone contributor comes out as its round-tripped wave
            else:
                out = torch.empty((2 * n_max,), dtype=torch.float32, device=stack.device)
                n_out = engine.ensemble_dev(stack.data_ptr(), k, n_max, self.algorithm, self.weights, out.data_ptr(), stream=stream)
                result = out[: 2 * n_out].view(1, 2, n_out)
            _, views = writer._host_planar_stems(result)
            writer._sync()
            outputs.append(self._write(path, stem_name, views[0], custom_output_names, file_rate))
        return outputs

    # ---- a batch of files: every member pools its files, one pooled combine ----------------------------------------------------
    HBM_SHARE = 0.4          # of the HBM free at the start of separate_many: what the stems of one run may take (estimated)

    def _stems_per_file(self, member):
        return stems_per_file(member)

    def _free_hbm(self):
        return free_hbm(self.members[-1].engine.device)

    def _runs(self, paths):
        """``pooled_runs`` over the stems of all members."""
        return pooled_runs(paths, self.pool_files, self._free_hbm, 8 * sum(self._stems_per_file(m) for m in self.members), self.HBM_SHARE)

    def separate_many(self, paths, custom_output_names=None):
        """``separate`` for a list of files with every member making ONE pooled call for all of them (``stems_dev_many``: the
        chunks, segments or patches of all files share the net passes) and ONE pooled device call combining the stems of all
        (file, stem group) pairs (``Engine.ensemble_batch_dev``).  Returns one list of output files per input, in order; the files
        are byte-identical to those of ``separate(path)`` called per path on the same members.

        * A file some member needs the host decoder for goes through the intermediate-file path alone, after the pooled files.
        * A file some member raised for fails alone: its result is an empty list, the exception is kept in
          ``self.batch_errors[index]`` and logged.
        * ``last_paths_taken[index]`` is "device", "files" or "failed".
        * A file whose stems some soundfile member would write in a format without a device round trip (``intermediate="writer"``:
          DOUBLE, PCM_U8, ...) goes through the intermediate-file path alone too.
        * What keeps the whole call off the device path (``via_files``, a soundfile writer unless ``intermediate="writer"``, a lossy output format, a member without
          ``stems_dev_many``) makes it the loop of ``separate`` per path.
        * Memory: the stems of all members for all files of a run are alive at once; ``paths`` is cut into consecutive runs (``_runs``).
        * Members see the files in list order, so the MDXC short-file rule evolves as in the loop.  Demucs members with
          ``shifts > 0`` draw their offsets from ``random`` member by member (each for all files), the loop file by file: with at
          most one such member the draws -- and the files -- are the same, with two or more they are assigned differently and the
          outputs need not match the loop's."""
        paths = list(paths)
        self.batch_errors = {}
        self.last_paths_taken = [None] * len(paths)
        results = [[] for _ in paths]
        why = self._device_path_refusal()
        if why is None and any(not hasattr(m, "stems_dev_many") for m in self.members):
            why = "a member has no pooled device-stem hook"
        if why is not None:
            if not self.via_files:
                self.logger.info(f"ensemble of {len(paths)} files one by one ({why})")
            for i, path in enumerate(paths):
                results[i] = self.separate(path, custom_output_names)
                self.last_paths_taken[i] = self.last_path_taken
            return results
        for run in self._runs(paths):
            self._separate_run(paths, run, custom_output_names, results)
        return results

    def _fail(self, i, path, e):
        self.logger.error(f"{path}: {e}")
        self.batch_errors[i] = e
        self.last_paths_taken[i] = "failed"

    def _separate_run(self, paths, run, custom_output_names, results):
        writer = self.members[-1]
        sub = [paths[i] for i in run]
        for path in sub:
            self.logger.info(f"Ensemble processing for file: {path}")
        pooled = [member.stems_dev_many(sub) for member in self.members]        # per member (stems per file, state per file)
        engine = writer.engine
        on_device, via_files = [], []              # (position in the run, groups) / positions
        for pos, i in enumerate(run):
            entries = [stems[pos] for stems, _ in pooled]
            error = next((e for e in entries if isinstance(e, BaseException)), None)
            if error is not None:
                self._fail(i, paths[i], error)
                continue
            needs_host = [index for index, e in enumerate(entries) if e is None]
            if needs_host:
                index = needs_host[0]
                self.logger.info(f"{paths[i]}: ensemble through intermediate files (member {index}, {self.members[index].model_name}, needs the host decoder)")
                via_files.append(pos)
                continue
            groups, refused = {}, None             # group name -> [(member index, device stem, layout, slot mode)], first-seen order
            for index, (member, stems) in enumerate(zip(self.members, entries)):
                member._restore_file(pooled[index][1][pos])
                names = self._group_names(member, [name for name, _, _ in stems])
                mode, why = self._slot_mode(member)        # of the state its own pass over this file left
                if mode is None:
                    refused = f"member {index}, {member.model_name}, {why}"
                    break
                for (_, tensor, layout), group in zip(stems, names):
                    groups.setdefault(group, []).append((index, tensor if tensor.is_contiguous() else tensor.contiguous(), layout, mode))
            if refused is not None:
                self.logger.info(f"{paths[i]}: ensemble through intermediate files ({refused})")
                via_files.append(pos)
                continue
            if any(t.device.index != engine.device for contributors in groups.values() for _, t, _, _ in contributors):
                self.logger.info(f"{paths[i]}: ensemble through intermediate files (members sit on different devices)")
                via_files.append(pos)
                continue
            on_device.append((pos, groups))
        for member in self.members:
            member._reset_file_state()
        # one pooled combine for every (file, group)
        jobs, outs, modes = [], [], []
        for pos, groups in on_device:
            for stem_name, contributors in groups.items():
                lengths = [t.shape[1] if layout == "planar" else t.shape[0] for _, t, layout, _ in contributors]
                out = self._result_buffer(contributors[0][1], 2 * max(lengths))
                outs.append(out)
                jobs.append(([(t.data_ptr(), n, layout) for (_, t, layout, _), n in zip(contributors, lengths)], out.data_ptr(), max(lengths)))
                modes.append([mode for _, _, _, mode in contributors])
        stream = writer._stream() if jobs else 0
        # "writer": the mode is each contributor's own (asx_ensemble_batch_modes_dev); otherwise one mode for the call, as ever
        how = {"modes": modes} if self.intermediate == "writer" else {"mode": self.intermediate}
        done = engine.ensemble_batch_dev(jobs, self.algorithm, self.weights, writer.normalization_threshold, writer.amplification_threshold,
                                         silent_below=_SILENT, stream=stream, **how) if jobs else []
        with writer._writing():
            j = 0
            for pos, groups in on_device:
                i = run[pos]
                writer._restore_file(pooled[-1][1][pos])      # what its own pass over this file left for the writer (bit depth, subtype, rate)
                file_rate = self._file_rate_of(writer, paths[i])
                outputs = []
                for stem_name, contributors in groups.items():
                    (n_out, live, peaks), out = done[j], outs[j]
                    j += 1
                    for (index, _, _, _), peak in zip(contributors, peaks):
                        if peak < _SILENT:
                            self.logger.warning(f"{stem_name}: the stem of member {index} ({self.members[index].model_name}) is silent, left out of the ensemble")
                    if live == 0:
                        continue
                    self.logger.info(f"Ensembling {live} stems for type: {stem_name}")
                    _, views = writer._host_planar_stems(out[: 2 * n_out].view(1, 2, n_out))
                    outputs.append(self._write(paths[i], stem_name, views[0], custom_output_names, file_rate))
                results[i] = outputs
                self.last_paths_taken[i] = self.last_path_taken = "device"
        writer._reset_file_state()
        del outs, pooled, on_device
        for pos in via_files:
            i = run[pos]
            try:
                results[i] = self._separate_via_files(paths[i], custom_output_names)
                self.last_paths_taken[i] = self.last_path_taken = "files"
            except Exception as e:
                self._fail(i, paths[i], e)

    @staticmethod
    def _result_buffer(like, numel):
        import torch
        return torch.empty((numel,), dtype=torch.float32, device=like.device)


class Ensembler:
    """Drop-in for audio_separator.separator.ensembler.Ensembler: same constructor, same ``ensemble(waveforms)``.  Stereo inputs
    are combined on the device (``Engine.ensemble``); anything else -- mono waves -- takes the numpy restatement of the
    wave-domain algorithms, and mismatched channel counts raise the reference's ValueError."""

    _engine = None           # one small engine for every instance that is not given one

    def __init__(self, logger, algorithm="avg_wave", weights=None, engine=None):
        self.logger = logger or logging.getLogger("audio_separator_amd")
        self.algorithm = algorithm
        self.weights = weights
        self.engine = engine

    def _get_engine(self):
        if self.engine is not None:
            return self.engine
        if Ensembler._engine is None:
            from .engine import Engine, MDXConfig
            Ensembler._engine = Engine(MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))   # the spectral edges need no net
        return Ensembler._engine

    def ensemble(self, waveforms):
        """ensembler.py:12-74."""
        if not waveforms:
            return None
        if len(waveforms) == 1:
            return waveforms[0]
        waveforms = [np.asarray(w) for w in waveforms]
        num_channels = waveforms[0].shape[0]
        if any(w.shape[0] != num_channels for w in waveforms):
            raise ValueError("All waveforms must have the same number of channels for ensembling.")
        if all(w.ndim == 2 for w in waveforms) and num_channels == 2:
            weights = effective_weights(self.weights, len(waveforms), self.logger)
            if self.weights is not None and not self.algorithm.startswith("avg_") and not np.all(weights == weights[0]):
                self.logger.warning(f"Weights are ignored for algorithm {self.algorithm}")
            self.logger.debug(f"Ensembling {len(waveforms)} waveforms using algorithm {self.algorithm}")
            return self._get_engine().ensemble(waveforms, self.algorithm, list(weights))
        return self._ensemble_numpy(waveforms)

    def _ensemble_numpy(self, waveforms):
        """The wave-domain algorithms as the reference computes them (ensembler.py:28-64), for inputs the engine does not take."""
        max_length = max(w.shape[1] for w in waveforms)
        waveforms = [np.pad(w, ((0, 0), (0, max_length - w.shape[1]))) if w.shape[1] < max_length else w for w in waveforms]
        weights = effective_weights(self.weights, len(waveforms), self.logger)
        if self.algorithm == "avg_wave":
            ensembled = np.zeros_like(waveforms[0])
            for w, weight in zip(waveforms, weights):
                ensembled += w * weight
            return ensembled / np.sum(weights)
        stacked = np.array(waveforms)
        if self.algorithm == "median_wave":
            return np.median(stacked, axis=0)
        if self.algorithm in ("min_wave", "max_wave"):
            pick = np.argmin if self.algorithm == "min_wave" else np.argmax
            idxs = np.expand_dims(pick(np.abs(stacked), 0), 0)
            return np.squeeze(np.take_along_axis(stacked, idxs, 0), axis=0)
        if self.algorithm in EnsembleSeparator.ALGORITHMS:
            raise ValueError(f"{self.algorithm} of {waveforms[0].shape[0]}-channel waves: the spectral ensembles run on the engine, "
                             "which takes stereo [2, N] waves")
        raise ValueError(f"Unknown ensemble algorithm: {self.algorithm}")
