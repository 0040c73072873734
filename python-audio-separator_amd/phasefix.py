"""Phase fix ("phase swapper") of two resident models: one model's STFT magnitudes on another's phases.

The community's remedy for the buzzing noise of the "fuller" Roformer instrumentals: keep the magnitudes of the fullness model's stem
(the *target*) and borrow the phases of a cleaner model's stem (the *source*, typically the instrumental complement of a vocal model),
more strongly towards high frequencies.  ``PhaseFixSeparator`` keeps both plugin instances (and their engines) loaded, takes the two
stems where ``stems_dev`` leaves them in HBM, forms the result there (``asx_phase_fix_batch_dev``, csrc/kernels_phasefix.h: one frame
launch and one fold) and has the target's writer encode it as a device-resident stem.

The rule is this project's own statement (include/asx.h): per channel, frame and bin of the librosa STFT(2048, hop),
with ``z = S conj(T)`` and ``delta = atan2(Im z, Re z)`` (0 where z == 0), ``O = T (cos(w delta) + j sin(w delta))`` -- a blend along
the shorter arc from the target's phase to the source's; ``w`` is 0 below ``low_hz``, ``high_weight`` above ``high_hz`` and linear
in between.  It is NOT the raw wrapped-angle blend of the community scripts.
"""
from __future__ import annotations

import logging
import os
import shutil
import tempfile

import numpy as np

from . import ensemble
from .workflow import ChainSeparator

N_FFT = 2048
N_BINS = N_FFT // 2 + 1     # ASX_PHASE_BINS
HOPS = (256, 512, 1024)


def bin_weights(sample_rate, low_hz=500.0, high_hz=5000.0, low_weight=0.0, high_weight=0.8) -> np.ndarray:
    """The blend per bin the engine is handed: float32 [1025], computed in float64.  Bin k sits at ``f = k * sample_rate / 2048``;
    ``low_weight`` for f < low_hz, ``high_weight`` for f > high_hz, linear in between; with ``low_hz == high_hz`` a bin exactly there
    takes ``high_weight``."""
    lo, hi, wl, wh = float(low_hz), float(high_hz), float(low_weight), float(high_weight)
    if lo > hi:
        raise ValueError(f"low_hz ({low_hz}) is above high_hz ({high_hz})")
    f32_max = float(np.finfo(np.float32).max)
    if not (abs(wl) <= f32_max and abs(wh) <= f32_max):       # (finite as float32 too; false for a NaN)
        raise ValueError(f"the weights must be finite, not {low_weight!r} and {high_weight!r}")
    f = np.arange(N_BINS, dtype=np.float64) * float(sample_rate) / N_FFT
    ramp = wl + (wh - wl) * ((f - lo) / (hi - lo)) if hi > lo else np.full(N_BINS, wh)
    ramp = np.where(f == hi, wh, ramp)           # (the upper end exactly, whatever the rounding of the line)
    return np.where(f < lo, wl, np.where(f > hi, wh, ramp)).astype(np.float32)


class _Tap:
    """``CommonSeparator._writer_tap`` for the host path: the array a member hands to ``write_audio`` for the named stem."""

    def __init__(self, stem):
        self.stem = stem.lower()
        self.seen, self.name, self.array = [], None, None

    def begin_stem(self, plugin, stem_name, stem_path, source):
        self.seen.append(stem_name)
        if stem_name.lower() == self.stem and self.array is None:
            plugin._sync()                       # (a pinned mirror of a device stem is filled by an asynchronous copy)
            self.name, self.array = stem_name, np.array(source, copy=True)

    def end_stem(self, plugin):
        pass

    def encoded(self, plugin, dev_stem, layout, n, encoded, subtype, peak):
        pass


class PhaseFixSeparator:
    OUTPUT_RATES = ("model", "input")

    def __init__(self, target, source, stem=("Instrumental", "Instrumental"), low_hz=500, high_hz=5000, low_weight=0.0, high_weight=0.8,
                 hop=512, output_rate="model", pool_files=None, logger=None):
        """``target`` / ``source``: two loaded plugin instances (MDXSeparator / MDXCSeparator / DemucsSeparator / VRSeparator, any pair);
        they and their engines stay resident across files.  ``stem``: (the target's stem, the source's stem), compared without case.
        ``low_hz`` / ``high_hz`` / ``low_weight`` / ``high_weight``: the blend per frequency (``bin_weights``); 500 / 5000 Hz are UVR's
        defaults, 0.8 the community notebook's, 0.0 below the lower cutoff this project's choice (the lows keep the target's phase).
        ``hop``: 256, 512 or 1024 samples between the frames of the 2048-point STFT.  ``output_rate``: "model" or "input" -- the result
        is written at the input file's sample rate and frame count, converted inside the target's writer.  ``pool_files``: files per
        pooled run of ``separate_many`` (None: EnsembleSeparator's memory rule).  Only the fixed stem is written, by the target's writer."""
        if target is source:
            raise ValueError("a phase fix needs two plugin instances: each member keeps its own per-file state")
        if isinstance(stem, str):
            stem = (stem, stem)
        stem = tuple(str(s) for s in stem)
        if len(stem) != 2:
            raise ValueError(f"stem is (the target's stem name, the source's stem name), not {stem!r}")
        if target.sample_rate != source.sample_rate:
            raise ValueError(f"the members differ in sample_rate ({target.sample_rate} and {source.sample_rate}): the stems are not resampled "
                             "between them")
        if ChainSeparator._device_of(target) != ChainSeparator._device_of(source):
            raise ValueError(f"the two engines are on different devices ({ChainSeparator._device_of(target)} and "
                             f"{ChainSeparator._device_of(source)}): the stems are combined in one device's memory")
        modes = [getattr(m, "asx_input_resample", "host") for m in (target, source)]
        if modes[0] != modes[1]:
            # a file at another rate would reach the members through different converters (or fail in one of them only)
            raise ValueError(f"the members differ in asx_input_resample: {modes}")
        for which, member, name in (("target", target, stem[0]), ("source", source, stem[1])):
            if getattr(member, "asx_output_rate", "model") == "input":
                raise ValueError(f"asx_output_rate='input' on the {which} is not supported in a phase fix: the stems and the combine stay at "
                                 "the model's rate; leave the members at 'model' and pass output_rate='input' to PhaseFixSeparator, which "
                                 "converts the result")
            if member.output_single_stem and member.output_single_stem.lower() != name.lower():
                raise ValueError(f"{which}.output_single_stem is {member.output_single_stem!r}, so the stem {name!r} would never be produced")
        if hop not in HOPS:
            raise ValueError(f"hop must be one of {HOPS}, not {hop!r}")
        if output_rate not in self.OUTPUT_RATES:
            raise ValueError(f"output_rate must be one of {self.OUTPUT_RATES}, not {output_rate!r}")
        if output_rate == "input":
            for m in (target, source):
                if getattr(m, "_output_rate_refusal", None):
                    raise ValueError(f"output_rate='input' is not supported with a {type(m).__name__} member: {m._output_rate_refusal}")
        if pool_files is not None and int(pool_files) < 1:
            raise ValueError(f"pool_files must be at least 1, not {pool_files!r}")
        self.weights = bin_weights(target.sample_rate, low_hz, high_hz, low_weight, high_weight)     # (refuses low_hz > high_hz, a weight that is not finite)
        self.target, self.source, self.stem, self.hop, self.output_rate = target, source, stem, int(hop), output_rate
        self.low_hz, self.high_hz, self.low_weight, self.high_weight = float(low_hz), float(high_hz), float(low_weight), float(high_weight)
        self.pool_files = None if pool_files is None else int(pool_files)
        self.model_filenames = [os.path.basename(m.model_path) if getattr(m, "model_path", None) else str(m.model_name) for m in (target, source)]
        self.logger = logger or target.logger or logging.getLogger("audio_separator_amd")
        self.last_path_taken = None                 # "device" | "files": the path the last input took
        self.last_paths_taken = []                  # separate_many: "device" | "files" | "failed" per input
        self.batch_errors = {}                      # separate_many: input index -> the exception that file raised

    # ---- shared pieces --------------------------------------------------------------------------------------------------------------
    def _device_path_refusal(self):
        """Why an input cannot take the device path, or None."""
        if os.environ.get("ASX_FILE_FASTPATH", "1") == "0":
            return "ASX_FILE_FASTPATH=0"
        try:
            import torch
            if not torch.cuda.is_available():
                return "there is no GPU"
        except Exception:
            return "there is no GPU"
        if any(not hasattr(m, "stems_dev") for m in (self.target, self.source)):
            return "a member has no device-stem hook"
        return None

    def _output_name(self, path, stem_name, custom_output_names):
        target = self.target
        ext = str(target.output_format).lower()
        lowered = {str(k).lower(): v for k, v in (custom_output_names or {}).items()}
        if stem_name.lower() in lowered:
            return f"{lowered[stem_name.lower()]}.{ext}"
        base = os.path.splitext(os.path.basename(path))[0]
        return f"{base}_({stem_name})_phasefix_{ensemble.model_slugs(self.model_filenames)}.{ext}"

    def _file_rate_of(self, path):
        """Under ``output_rate`` = "input": (sample rate, frames) of the file the target has just loaded; None under "model"."""
        return ensemble.file_rate_of(self.target, path) if self.output_rate == "input" else None

    @staticmethod
    def _pick(stems, name, who, path):
        """The entry of ``stems`` ([(stem name, tensor, layout)]) called ``name``, without case."""
        for entry in stems:
            if entry[0].lower() == name.lower():
                return entry
        raise ValueError(f"{name!r} is not a stem {who.model_name} produces for {path}: it has {[e[0] for e in stems]}")

    @staticmethod
    def _length(tensor, layout):
        return tensor.shape[1] if layout == "planar" else tensor.shape[0]

    def _write(self, path, fname, source, file_rate, device_stem=None):
        """The target's writer on the result: ``source`` [n, 2], or -- ``device_stem`` a planar CUDA tensor [2, n] -- a stand-in of that
        shape registered against the tensor, which the writer then normalises and encodes where it is."""
        target = self.target
        target.audio_file_path = path
        target._output_rate_override = file_rate
        try:
            if device_stem is not None:
                target._dev_stems[id(source)] = (source, device_stem, None, "planar")
            try:
                target.write_audio(fname, source)
            finally:
                target._dev_stems.pop(id(source), None)
        finally:
            target._output_rate_override = None
        return fname

    def _write_device(self, path, fname, result, n, file_rate):
        target = self.target
        if fname.lower().endswith(".flac") or (target.use_soundfile and not target._soundfile_on_device(fname)):
            # The result comes back once, as the host path's does, and the writer takes it as a host array.  FLAC: the writers leave the
            # MD5 of STREAMINFO unset for samples that never reached the host, so only this way are the two paths' files the same bytes
            # (and the stream carries its checksum).  The soundfile writer on the host reads the array itself.
            target._sync()
            return self._write(path, fname, np.ascontiguousarray(result.t().cpu().numpy()), file_rate)
        stand_in = np.broadcast_to(np.float32(0), (n, 2))          # stands for the shape only: the writer reads the device tensor
        return self._write(path, fname, stand_in, file_rate, device_stem=result)

    def _job(self, t_entry, s_entry):
        """(engine job, result tensor [2, n], n) for the picked stems of one file"""
        import torch
        (_, t, t_layout), (_, s, s_layout) = t_entry, s_entry
        t = t if t.is_contiguous() else t.contiguous()
        s = s if s.is_contiguous() else s.contiguous()
        n, n_src = self._length(t, t_layout), self._length(s, s_layout)
        if n < 1:
            raise ValueError("the target's stem is empty")
        out = torch.empty((2, n), dtype=torch.float32, device=t.device)
        return ((t.data_ptr(), t_layout, n), (s.data_ptr(), s_layout, n_src), (out.data_ptr(), "planar")), out, n, (t, s)

    # ---- one file ---------------------------------------------------------------------------------------------------------------------
    def separate(self, audio_file_path, custom_output_names=None):
        """One input through both members and the phase fix -> [the name of the fixed stem's file] (as for any stem, the writer leaves a
        silent result out)."""
        path = audio_file_path
        self.logger.info(f"Phase fix for file: {path}")
        why = self._device_path_refusal()
        files = None
        if why is None:
            files, why = self._separate_on_device(path, custom_output_names)
        if files is None:
            self.logger.info(f"{path}: phase fix through the members' host arrays ({why})")
            files = self._separate_via_files(path, custom_output_names)
            self.last_path_taken = "files"
        else:
            self.last_path_taken = "device"
        return files

    def _separate_on_device(self, path, custom_output_names):
        """(files, None), or (None, why) when this input needs the host path (a member could not keep its stems on the device)."""
        target, source = self.target, self.source
        picked = []
        for member, name in ((target, self.stem[0]), (source, self.stem[1])):
            stems = member.stems_dev(path)
            if member is target:
                file_rate = self._file_rate_of(path)
            member.clear_file_specific_paths()
            if stems is None:
                return None, f"{member.model_name} needs the host decoder"
            picked.append(self._pick(stems, name, member, path))
        if any(e[1].device.index != target.engine.device for e in picked):
            return None, "the members' stems sit on different devices"
        job, result, n, _keep = self._job(*picked)
        target.engine.phase_fix_batch_dev([job], self.weights, self.hop, stream=target._stream())
        fname = self._output_name(path, picked[0][0], custom_output_names)
        with target._writing():
            self._write_device(path, fname, result, n, file_rate)
        target.clear_file_specific_paths()
        return [fname], None

    def _separate_via_files(self, path, custom_output_names):
        """Each member's ``separate`` into a temporary directory with a tap on its writer, ``Engine.phase_fix`` on the two arrays the
        taps kept, the target's ``write_audio``: the same launches on the same samples, so the file is the device path's byte for byte."""
        target, source = self.target, self.source
        temp_dir = tempfile.mkdtemp(prefix="audio-separator-phasefix-")
        taps = []
        try:
            for member, name in ((target, self.stem[0]), (source, self.stem[1])):
                tap = _Tap(name)
                saved = member.output_dir
                member.output_dir, member._writer_tap = temp_dir, tap
                try:
                    member.separate(path, None)
                    if member is target:
                        file_rate = self._file_rate_of(path)
                    member.clear_gpu_cache()
                    member.clear_file_specific_paths()
                finally:
                    member.output_dir, member._writer_tap = saved, None
                if tap.array is None:
                    raise ValueError(f"{name!r} is not a stem {member.model_name} produces for {path}: it has {tap.seen}")
                taps.append(tap)
        finally:
            shutil.rmtree(temp_dir, ignore_errors=True)
        t, s = (np.ascontiguousarray(tap.array, np.float32) for tap in taps)
        if t.ndim != 2 or t.shape[1] != 2 or s.ndim != 2 or s.shape[1] != 2 or t.shape[0] < 1:
            raise ValueError(f"the phase fix takes stereo stems [n, 2] with n >= 1, not {t.shape} and {s.shape}")
        result = target.engine.phase_fix(t, s, self.weights, self.hop)
        fname = self._output_name(path, taps[0].name, custom_output_names)
        self._write(path, fname, result, file_rate)
        target.clear_file_specific_paths()
        return [fname]

    # ---- a batch of files: each member pools its files, one pooled phase fix ------------------------------------------------------------
    def separate_many(self, paths, custom_output_names=None):
        """``separate`` for a list of files: each member makes ONE pooled call for the files of a run (``stems_dev_many``), then ONE
        ``phase_fix_batch_dev`` call serves them.  Returns one list of output files per input, in order; the files are byte-identical
        to those of ``separate(path)`` called per path.  A file some member raised for fails alone (an empty list,
        ``batch_errors[index]``); one a member needs the host decoder for takes the host path alone, after the pooled files;
        ``last_paths_taken[index]`` is "device", "files" or "failed"."""
        paths = list(paths)
        self.batch_errors = {}
        self.last_paths_taken = [None] * len(paths)
        results = [[] for _ in paths]
        why = self._device_path_refusal()
        if why is None and any(not hasattr(m, "stems_dev_many") for m in (self.target, self.source)):
            why = "a member has no pooled device-stem hook"
        if why is not None:
            self.logger.info(f"phase fix of {len(paths)} files one by one ({why})")
            for i, path in enumerate(paths):
                try:
                    results[i] = self.separate(path, custom_output_names)
                    self.last_paths_taken[i] = self.last_path_taken
                except Exception as e:
                    self._fail(i, path, e)
            return results
        members = (self.target, self.source)
        per_frame = 8 * (sum(ensemble.stems_per_file(m) for m in members) + 1)        # (+ the result)
        for run in ensemble.pooled_runs(paths, self.pool_files, lambda: ensemble.free_hbm(self.target.engine.device), per_frame,
                                        ensemble.EnsembleSeparator.HBM_SHARE):
            self._separate_run(paths, run, custom_output_names, results)
        return results

    def _fail(self, i, path, e):
        self.logger.error(f"{path}: {e}")
        self.batch_errors[i] = e
        self.last_paths_taken[i] = "failed"

    def _separate_run(self, paths, run, custom_output_names, results):
        target, source = self.target, self.source
        sub = [paths[i] for i in run]
        for path in sub:
            self.logger.info(f"Phase fix for file: {path}")
        pooled = [member.stems_dev_many(sub) for member in (target, source)]         # per member (stems per file, state per file)
        planned, via_files = [], []                # (position in the run, job, result, n, stem name) / positions
        for pos, i in enumerate(run):
            entries = [stems[pos] for stems, _ in pooled]
            error = next((e for e in entries if isinstance(e, BaseException)), None)
            if error is not None:
                self._fail(i, paths[i], error)
                continue
            needs_host = [m for m, e in zip((target, source), entries) if e is None]
            if needs_host:
                self.logger.info(f"{paths[i]}: phase fix through the members' host arrays ({needs_host[0].model_name} needs the host decoder)")
                via_files.append(pos)
                continue
            try:
                picked = [self._pick(e, name, m, paths[i]) for e, name, m in zip(entries, self.stem, (target, source))]
                if any(e[1].device.index != target.engine.device for e in picked):
                    self.logger.info(f"{paths[i]}: phase fix through the members' host arrays (the members' stems sit on different devices)")
                    via_files.append(pos)
                    continue
                job, result, n, keep = self._job(*picked)
            except Exception as e:
                self._fail(i, paths[i], e)
                continue
            planned.append((pos, job, result, n, picked[0][0], keep))
        for member in (target, source):
            member._reset_file_state()
        if planned:
            target.engine.phase_fix_batch_dev([p[1] for p in planned], self.weights, self.hop, stream=target._stream())
        with target._writing():
            for pos, _, result, n, stem_name, _keep in planned:
                i = run[pos]
                target._restore_file(pooled[0][1][pos])       # what its own pass over this file left for the writer (bit depth, subtype, rate)
                try:
                    fname = self._output_name(paths[i], stem_name, custom_output_names)
                    self._write_device(paths[i], fname, result, n, self._file_rate_of(paths[i]))
                    results[i] = [fname]
                    self.last_paths_taken[i] = self.last_path_taken = "device"
                except Exception as e:
                    self._fail(i, paths[i], e)
        target._reset_file_state()
        del planned, pooled
        for pos in via_files:
            i = run[pos]
            try:
                results[i] = self._separate_via_files(paths[i], custom_output_names)
                self.last_paths_taken[i] = self.last_path_taken = "files"
            except Exception as e:
                self._fail(i, paths[i], e)
