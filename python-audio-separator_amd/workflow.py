"""Chains of two resident models: the second one runs on a stem of the first.

The usual ways to combine models are an ensemble (ensemble.py: several models on the same input, their stems combined) and a
chain: a karaoke model splits the vocal stem of a vocal / instrumental model into lead and backing vocals, a de-reverb model
cleans a vocal stem, an "instrumental + backing vocals" track is mixed from stems of both.  ``ChainSeparator`` keeps the two
plugin instances (and their engines) loaded and has ONE contract, the literal flow through the stem's file::

    a = first.separate(path)
    b = then.separate(os.path.join(first.output_dir, <the file of a that holds `stem`>))
    result = a + b (+ mix-downs)

* ``handoff="file"`` (the default) gives exactly the files of that flow, on either path the call can take.  On the device path
  the input is read and decoded once, ``first`` demixes once and writes its files with its own writer, and the buffer that writer
  encodes the chosen stem into ON THE DEVICE (int16 from ``asx_pcm16*_dev``, or the file's own PCM_16 / PCM_24 / PCM_32 / FLOAT
  bytes from ``asx_pcm_encode_dev`` under ``use_soundfile``) is decoded where it is (``asx_pcm_decode_dev``) into the planar mix a
  reader of the stem's file would get, and handed to ``then`` through the door of ``CommonSeparator`` (``_inject_mix``) together
  with the per-file state a decode of that file would have left.  The round trip through the file is reproduced by construction:
  the same encoder output serves the file and the hand-off.  Where that is not possible the call IS the literal flow
  (``last_path_taken == "files"``).
* ``handoff="float"`` hands ``then`` the stem after the writer's normalise and nothing else: float32, never quantised, so no
  16-bit rounding sits between the two models.  ``then``'s writer keeps the ORIGINAL input's sample format.
* ``mixdowns`` are weighted sums of stems of both stages, formed in HBM by ``asx_mixdown_batch_dev`` (csrc/kernels_mix.h) and
  written by ``then``'s writer as device-resident stems.  ``then`` heard the stem scaled by ``g`` (``last_handoff_gain``), so its
  stems enter with ``float32(w / g)``: a mix-down is at the first stage's scale.
"""
from __future__ import annotations

import logging
import os

import numpy as np

_SILENT = 1e-6          # write_audio writes no file for a stem whose peak after normalisation is below this
_LOSSLESS = ("wav", "flac")
MAX_TERMS = 8           # ASX_MIX_MAX_K


def then_weight(weight, gain) -> np.float32:
    """The weight a stem of ``then`` enters a mix-down with: ``float32(w / g)``, the quotient taken in float64."""
    return np.float32(np.float64(weight) / np.float64(gain))


def mixdown_host(sources, n_out=None) -> np.ndarray:
    """The mix-down rule on host arrays, numpy float32: ``sources`` = [(array [n, 2], weight)] -> [n_out, 2] (``n_out``: the longest
    source unless given); ``acc = fl(w_0 x_0)``, ``acc = fl(acc + fl(w_k x_k))`` in list order, a shorter source zero-extended.
    What ``asx_mixdown_batch_dev`` computes, bit for bit."""
    sources = [(np.asarray(a, np.float32), np.float32(w)) for a, w in sources]
    if not 1 <= len(sources) <= MAX_TERMS:
        raise ValueError(f"a mix-down takes 1 .. {MAX_TERMS} terms, not {len(sources)}")
    if n_out is None:
        n_out = max(a.shape[0] for a, _ in sources)
    acc = None
    for a, w in sources:
        x = np.zeros((n_out, 2), np.float32)
        m = min(n_out, a.shape[0])
        x[:m] = a[:m]
        term = w * x
        acc = term if acc is None else acc + term
    return acc


def _vr_format(subtype):
    """(wav_subtype, input_bit_depth) VRSeparator._probe_vr_format derives from a file's subtype."""
    if subtype and "24" in subtype:
        return "PCM_24", 24
    if subtype and "32" in subtype:
        return "PCM_32", 32
    return "PCM_16", 16


class _Tap:
    """The listener a stage carries for the span of a chain call (``CommonSeparator._writer_tap``): which stems the plugin handed
    to its writer for which input, and -- for the stems named in ``keep`` and the handed stem -- what the device writers saw."""

    def __init__(self, keep=(), handed=None, handoff=None, capture=True):
        self.keep = {k.lower() for k in keep}
        self.handed = handed.lower() if handed else None
        self.handoff, self.capture = handoff, capture
        self.files = {}                      # audio_file_path -> {"state": per-file state, "stems": [entry]}
        self.current = None

    def begin_stem(self, plugin, stem_name, stem_path, source):
        rec = self.files.get(plugin.audio_file_path)
        if rec is None:
            state = {k: getattr(plugin, k, None) for k in plugin._PER_FILE if k not in ("_file_mix", "_mix_scale")}
            rec = self.files[plugin.audio_file_path] = {"state": state, "stems": []}
        wanted = stem_name.lower() in self.keep or stem_name.lower() == self.handed
        self.current = {"name": stem_name, "path": stem_path, "source": source if wanted else None, "wanted": wanted, "peak": None,
                        "n": None, "dev": None, "layout": None, "encoded": None, "subtype": None, "gain": 1.0}
        rec["stems"].append(self.current)

    def end_stem(self, plugin):
        self.current = None

    def encoded(self, plugin, dev_stem, layout, n, encoded, subtype, peak):
        e = self.current
        if e is None or not e["wanted"] or not self.capture:
            return
        e["peak"], e["n"] = float(peak), int(n)
        if e["name"].lower() in self.keep or self.handoff == "float":
            e["dev"], e["layout"] = dev_stem, layout
        if e["name"].lower() == self.handed:
            if peak >= _SILENT:              # (a silent stem ends the chain; under a minimum peak its factor would not be finite)
                e["gain"] = plugin.engine.normalize_scale_dev(dev_stem.data_ptr(), 2 * int(n), plugin.normalization_threshold,
                                                              plugin.amplification_threshold, stream=plugin._stream())
            if self.handoff == "file":
                e["encoded"], e["subtype"] = encoded, subtype

    def entry(self, path, stem_name):
        rec = self.files.get(path)
        for e in (rec["stems"] if rec else ()):
            if e["name"].lower() == stem_name.lower():
                return e
        return None


class ChainSeparator:
    HANDOFFS = ("file", "float")

    def __init__(self, first, then, stem, handoff="file", mixdowns=None, logger=None):
        """``first`` / ``then``: loaded plugin instances (MDXSeparator / MDXCSeparator / DemucsSeparator / VRSeparator, any pair); they
        and their engines stay resident across files.  ``stem``: the stem of ``first`` that becomes the input of ``then`` (compared
        without case, as ``output_single_stem`` is).  ``handoff``: "file" or "float" (module docstring).  ``mixdowns``:
        ``{name: [(stage, stem name, weight), ...]}``, ``stage`` "first" or "then", at most 8 terms each."""
        if handoff not in self.HANDOFFS:
            raise ValueError(f"handoff must be one of {self.HANDOFFS}, not {handoff!r}")
        if first is then:
            raise ValueError("a chain needs two plugin instances: each stage keeps its own per-file state")
        if first.sample_rate != then.sample_rate:
            raise ValueError(f"the stages differ in sample_rate ({first.sample_rate} and {then.sample_rate}): the handed stem is not resampled "
                             "between them")
        for which, plugin in (("first", first), ("then", then)):
            if getattr(plugin, "asx_output_rate", "model") == "input":
                raise ValueError(f"asx_output_rate='input' on the {which} stage is not supported in a chain: the hand-off and the mix-downs "
                                 "live at the model's rate (a chain-level output rate is out of scope)")
        if first.output_single_stem and first.output_single_stem.lower() != str(stem).lower():
            raise ValueError(f"first.output_single_stem is {first.output_single_stem!r}, so the stem {stem!r} would never be produced")
        if self._device_of(first) != self._device_of(then):
            raise ValueError(f"the two engines are on different devices ({self._device_of(first)} and {self._device_of(then)}): the stem is "
                             "handed over in one device's memory")
        if handoff == "float":
            if not then._takes_device_mix():
                raise ValueError(f"handoff='float' needs a second stage that takes a device-resident mix; {then.model_name} decodes its "
                                 "inputs on the host")
            if getattr(then, "segments_enabled", True) is False:
                raise ValueError("handoff='float' needs a second stage that demixes on the device; segments_enabled=False combines on the host")
        self.mixdowns = {}
        for name, terms in (mixdowns or {}).items():
            terms = [tuple(t) for t in terms]
            if not 1 <= len(terms) <= MAX_TERMS:
                raise ValueError(f"mix-down {name!r}: {len(terms)} terms (1 .. {MAX_TERMS})")
            for t in terms:
                if len(t) != 3 or t[0] not in ("first", "then"):
                    raise ValueError(f"mix-down {name!r}: a term is (stage, stem name, weight) with stage 'first' or 'then', not {t!r}")
                if not np.isfinite(np.float32(t[2])):
                    raise ValueError(f"mix-down {name!r}: the weight of {t[1]!r} is not finite")
            self.mixdowns[name] = [(s, str(n), float(w)) for s, n, w in terms]
        self.first, self.then, self.stem, self.handoff = first, then, str(stem), handoff
        self.logger = logger or first.logger or logging.getLogger("audio_separator_amd")
        self.last_path_taken = None                 # "device" | "files": the path the last input took
        self.last_paths_taken = []                  # separate_many: "device" | "files" | "failed" per input
        self.last_handoff_gain = 1.0                # g: the float32 factor the writer's normalise applied to the handed stem
        self.batch_errors = {}                      # separate_many: input index -> the exception that file raised

    @staticmethod
    def _device_of(plugin):
        eng = getattr(plugin, "engine", None)
        if eng is not None and hasattr(eng, "device"):
            return int(eng.device)
        text = str(getattr(plugin, "torch_device", None) or "cuda:0")
        return int(text.split(":")[1]) if ":" in text else 0

    # ---- what keeps a call off the device path --------------------------------------------------------------------------------
    def _device_path_refusal(self):
        """Why the stem cannot be handed over in HBM, or None.  (That ``first``'s device decoder does not take a file shows only
        when it is loaded: ``_handoff`` sees that the device writers never met the stem.)"""
        first = self.first
        if os.environ.get("ASX_FILE_FASTPATH", "1") == "0":
            return "ASX_FILE_FASTPATH=0"
        try:
            import torch
            if not torch.cuda.is_available():
                return "there is no GPU"
        except Exception:
            return "there is no GPU"
        fmt = str(first.output_format).lower()
        if fmt not in _LOSSLESS:
            return f"output_format {first.output_format} is not one of {_LOSSLESS} (the stem's file would not be lossless)"
        if first.use_soundfile and fmt == "flac":
            return "use_soundfile writes FLAC stems from int32 containers, which have no device round trip"
        if first.use_soundfile and not first._soundfile_on_device(f"stem.{fmt}"):
            return "the first stage writes its stems with soundfile on the host"
        if not self.then._takes_device_mix():
            return f"{self.then.model_name} decodes its inputs on the host"
        return None

    def _known_stems(self):
        """The stems of ``first`` where they are known before a file is loaded (Demucs and MDXC know them after the demix)."""
        first = self.first
        if hasattr(first, "demucs_source_map") or hasattr(first, "_stem_plan"):
            return None
        return [first.primary_stem_name, first.secondary_stem_name]

    def _then_state(self, entry, original):
        """The per-file state a decode of the stem's file would have left on ``then`` ("file"), or the original input's sample format
        around the stem's length ("float")."""
        first, then = self.first, self.then
        n, rate = entry["n"], first.sample_rate
        if self.handoff == "float":
            subtype, depth = original.get("input_subtype"), original.get("input_bit_depth")
            vr_subtype = original.get("input_audio_subtype") or subtype
        else:
            if first.use_soundfile:
                subtype = entry["subtype"]
            else:
                depth = original.get("input_bit_depth")       # (this file's, as first's writer saw it)
                depth = depth if depth is not None else 16
                if str(first.output_format).lower() == "flac":
                    subtype = "PCM_24" if depth in (24, 32) else "PCM_16"
                else:
                    subtype = {16: "PCM_16", 24: "PCM_24", 32: "PCM_32"}.get(depth, "PCM_16")
            depth = 16 if subtype == "PCM_16" else (24 if subtype == "PCM_24" else 32)
            vr_subtype = subtype
        state = {"_file_seconds": n / float(rate), "_file_rate": rate, "_file_frames": n}
        if hasattr(then, "_probe_vr_format"):
            wav_subtype, vr_depth = _vr_format(vr_subtype)
            state.update(wav_subtype=wav_subtype, input_audio_subtype=vr_subtype, input_bit_depth=vr_depth)
        else:
            state.update(input_subtype=subtype, input_bit_depth=depth)
        return state

    def _handoff(self, path, tap, refusal):
        """After ``first`` wrote the files of ``path``: find the stem, inject it into ``then`` where it is still in HBM.  Returns
        (the stem's file as ``then`` will be given it, "device" | "files", why not the device)."""
        first, then = self.first, self.then
        rec = tap.files.get(path)
        entry = tap.entry(path, self.stem)
        if entry is None:
            names = [e["name"] for e in rec["stems"]] if rec else []
            raise ValueError(f"{self.stem!r} is not a stem {first.model_name} writes for {path}: it wrote {names}")
        stem_file = os.path.join(first.output_dir, entry["path"]) if first.output_dir else entry["path"]
        self.last_handoff_gain = 1.0
        seen = entry["peak"] is not None              # the device writers met the stem
        on_device = seen and (entry["encoded"] is not None if self.handoff == "file" else entry["dev"] is not None)
        if (seen and entry["peak"] < _SILENT) or (not seen and not os.path.isfile(stem_file)):
            raise ValueError(f"the {entry['name']} stem of {path} is silent: {first.model_name} wrote no file for it, the chain ends here")
        thr, amp = first.normalization_threshold, first.amplification_threshold
        if on_device:
            import torch
            n, eng, st = entry["n"], first.engine, first._stream()
            self.last_handoff_gain = float(entry["gain"])
            if self.handoff == "file":
                mix = torch.empty((2, n), dtype=torch.float32, device=entry["encoded"].device)
                peak = eng.pcm_decode_dev(entry["encoded"].data_ptr(), n, 2, entry["subtype"], mix.data_ptr(), stream=st)
                entry["encoded"] = None
            else:
                dev = entry["dev"]
                mix = dev.clone() if entry["layout"] == "planar" else dev.t().contiguous()
                eng.normalize_dev(mix.data_ptr(), 2 * n, thr, amp, stream=st)
                peak = entry["peak"]
                if entry["name"].lower() not in tap.keep:
                    entry["dev"] = None
            then._inject_mix(stem_file, mix, self._then_state(entry, rec["state"]), peak)
            return stem_file, "device", None
        why = refusal or f"the first stage's device writer never saw the {entry['name']} stem (its decoder did not take the file)"
        if self.handoff == "float":
            # no file holds the unquantised stem: it is normalised on the host array the writer was handed, and uploaded
            import torch
            a = np.array(entry["source"], np.float32, copy=True)
            peak_before = float(np.abs(a).max()) if a.size else 0.0
            self.last_handoff_gain = first._normalize_factor(peak_before) if peak_before > 0 else 1.0
            a = first.engine.normalize(np.ascontiguousarray(a), thr, amp)
            entry["n"] = a.shape[0]
            mix = torch.from_numpy(np.ascontiguousarray(a.T)).to(first._torch_device())
            then._inject_mix(stem_file, mix, self._then_state(entry, rec["state"]), float(np.abs(a).max()) if a.size else 0.0)
        else:
            self.last_handoff_gain = self._gain_of_host(entry)
        return stem_file, "files", why

    def _gain_of_host(self, entry):
        a = np.asarray(entry["source"]) if entry["source"] is not None else None
        if a is None or not a.size or a.dtype == np.int16:
            return 1.0
        peak = float(np.abs(a).max())
        return self.first._normalize_factor(peak) if peak > 0 else 1.0

    # ---- mix-downs --------------------------------------------------------------------------------------------------------------
    def _mixdown_name(self, base, name, custom_output_names):
        then = self.then
        ext = str(then.output_format).lower()
        if custom_output_names:
            lowered = {k.lower(): v for k, v in custom_output_names.items()}
            if name.lower() in lowered:
                return f"{then.sanitize_filename(lowered[name.lower()])}.{ext}"
        s = then.sanitize_filename
        return f"{s(base)}_({s(name)})_{s(str(self.first.model_name))}+{s(str(self.then.model_name))}.{ext}"

    def _mixdown_terms(self, name, path, stem_file, tap1, tap2, gain):
        terms = []
        for stage, stem, w in self.mixdowns[name]:
            e = tap1.entry(path, stem) if stage == "first" else tap2.entry(stem_file, stem)
            if e is None:
                raise ValueError(f"mix-down {name!r}: {stem!r} is not a stem the {stage} stage wrote for {path}")
            terms.append((e, np.float32(w) if stage == "first" else then_weight(w, gain)))
        return terms

    def _write_mixdowns(self, items, custom_output_names, tap1, tap2):
        """``items``: [(index, path, stem file, g)] of the inputs both stages served.  Every mix-down whose terms are all still in HBM
        is formed there -- ONE launch for all of them -- and written by ``then``'s writer as a device-resident stem; the others are
        formed with numpy float32 from the arrays the stages handed to ``write_audio``.  Returns {index: [file names]}, {index: error}."""
        then = self.then
        out, errors, jobs, plans = {}, {}, [], []
        for i, path, stem_file, gain in items:
            base = os.path.splitext(os.path.basename(path))[0]
            try:
                for name in self.mixdowns:
                    terms = self._mixdown_terms(name, path, stem_file, tap1, tap2, gain)
                    fname = self._mixdown_name(base, name, custom_output_names)
                    if all(e["dev"] is not None for e, _ in terms):
                        import torch
                        n_out = max(e["n"] for e, _ in terms)
                        mixed = torch.empty((2, n_out), dtype=torch.float32, device=terms[0][0]["dev"].device)
                        jobs.append(([(e["dev"].data_ptr(), e["layout"], e["n"], float(w)) for e, w in terms], mixed.data_ptr(), "planar", n_out))
                        plans.append((i, stem_file, fname, mixed, n_out, terms))
                    else:
                        plans.append((i, stem_file, fname, mixdown_host([(np.asarray(e["source"]), w) for e, w in terms]), None, terms))
            except Exception as e:
                errors[i] = e
        if jobs:
            then.engine.mixdown_batch_dev(jobs, stream=then._stream())
        keep = {k: getattr(then, k, None) for k in then._PER_FILE}
        try:
            for i, stem_file, fname, mixed, n_out, _terms in plans:
                if i in errors:
                    continue
                rec = tap2.files.get(stem_file)
                for k, v in (rec["state"] if rec else {}).items():
                    setattr(then, k, v)
                try:
                    with then._writing():
                        if n_out is None:
                            then.write_audio(fname, mixed)
                        else:
                            stand_in = np.broadcast_to(np.float32(0), (n_out, 2))      # stands for the shape only: the writer reads the device tensor
                            then._dev_stems[id(stand_in)] = (stand_in, mixed, None, "planar")
                            try:
                                then.write_audio(fname, stand_in)
                            finally:
                                then._dev_stems.pop(id(stand_in), None)
                    out.setdefault(i, []).append(fname)
                except Exception as e:
                    errors[i] = e
        finally:
            for k, v in keep.items():
                setattr(then, k, v)
        return out, errors

    # ---- the calls ------------------------------------------------------------------------------------------------------------------
    def _taps(self, refusal):
        keep1 = [s for terms in self.mixdowns.values() for stage, s, _ in terms if stage == "first"]
        keep2 = [s for terms in self.mixdowns.values() for stage, s, _ in terms if stage == "then"]
        capture = refusal is None
        return (_Tap(keep1, handed=self.stem, handoff=self.handoff, capture=capture), _Tap(keep2, capture=capture))

    def _check_stem_known(self):
        known = self._known_stems()
        if known is not None and self.stem.lower() not in [str(k).lower() for k in known]:
            raise ValueError(f"{self.stem!r} is not a stem of {self.first.model_name}: it has {known}")

    def separate(self, audio_file_path, custom_output_names=None):
        """One input through both stages: the files of ``first``, then those of ``then`` on the handed stem, then the mix-downs."""
        results = self._run([audio_file_path], custom_output_names, pooled=False)
        self.last_path_taken = self.last_paths_taken[0]
        if 0 in self.batch_errors:
            raise self.batch_errors[0]
        return results[0]

    def separate_many(self, paths, custom_output_names=None):
        """``separate`` for a list of inputs: ``first`` through its pooled call (one engine call for all files), the hand-offs, ``then``
        through its pooled call over all handed stems.  The files are byte-identical to a loop of ``separate``.  An input that fails
        at either stage fails alone: its result is an empty list -- or the first stage's files where those were written -- and
        ``batch_errors[i]`` holds the exception (the rule of ``CommonSeparator._separate_many``)."""
        paths = list(paths)
        if len(set(paths)) != len(paths):            # the records of the two stages are kept per path
            results, errors, taken = [], {}, []
            for i, p in enumerate(paths):
                r = self._run([p], custom_output_names, pooled=False)
                results.append(r[0])
                taken.append(self.last_paths_taken[0])
                if 0 in self.batch_errors:
                    errors[i] = self.batch_errors[0]
            self.batch_errors, self.last_paths_taken = errors, taken
        else:
            results = self._run(paths, custom_output_names, pooled=True)
        self.last_path_taken = next((t for t in reversed(self.last_paths_taken) if t != "failed"), None)
        return results

    def _stage(self, plugin, paths, custom_output_names, pooled):
        """``plugin.separate`` over ``paths`` -- its pooled call where it has one -- with the fail-alone rule: ([file names per path],
        {index: exception}).  A single input raises as ``separate`` does."""
        if pooled and hasattr(plugin, "separate_many"):
            lists = plugin.separate_many(paths, custom_output_names)
            return [list(x) for x in lists], dict(getattr(plugin, "batch_errors", {}) or {})
        lists, errors = [], {}
        for i, p in enumerate(paths):
            try:
                lists.append(list(plugin.separate(p, custom_output_names)))
            except Exception as e:
                if not pooled:
                    raise
                self.logger.error(f"{p}: {e}")
                lists.append([])
                errors[i] = e
        return lists, errors

    def _run(self, paths, custom_output_names, pooled):
        first, then = self.first, self.then
        self._check_stem_known()
        refusal = self._device_path_refusal()
        if refusal is not None:
            self.logger.info(f"chain through the stem's file ({refusal})")
        tap1, tap2 = self._taps(refusal)
        results = [[] for _ in paths]
        self.batch_errors = {}
        taken = ["failed"] * len(paths)
        first._writer_tap, then._writer_tap = tap1, tap2
        try:
            try:
                a_lists, errors = self._stage(first, paths, custom_output_names, pooled)
            except Exception as e:
                if pooled:
                    raise
                self.batch_errors[0] = e
                self.last_paths_taken = taken
                return results
            self.batch_errors.update(errors)
            handed = []                               # (index, path, stem file, g)
            for i, path in enumerate(paths):
                results[i] = a_lists[i]
                if i in errors:
                    continue
                try:
                    stem_file, where, why = self._handoff(path, tap1, refusal)
                except Exception as e:
                    self.logger.error(f"{path}: {e}")
                    self.batch_errors[i] = e
                    continue
                if where == "files" and refusal is None:
                    self.logger.info(f"{path}: chain through the stem's file ({why})")
                taken[i] = where
                handed.append((i, path, stem_file, self.last_handoff_gain))
            if handed:
                try:
                    b_lists, errors = self._stage(then, [h[2] for h in handed], custom_output_names, pooled)
                except Exception as e:
                    if pooled:
                        raise
                    self.batch_errors[handed[0][0]] = e
                    taken[handed[0][0]] = "failed"
                    self.last_paths_taken = taken
                    return results
                left = set((then._injected or {}).keys())      # a mix ``then`` did not take: it read the stem's file instead
                served = []
                for j, (i, path, stem_file, gain) in enumerate(handed):
                    if j in errors:
                        self.batch_errors[i] = errors[j]
                        taken[i] = "failed"
                        continue
                    if stem_file in left and taken[i] == "device":
                        taken[i] = "files"
                        self.logger.info(f"{path}: chain through the stem's file ({then.model_name} took the file, not the device mix)")
                    results[i] = results[i] + b_lists[j]
                    served.append((i, path, stem_file, gain))
                if self.mixdowns and served:
                    written, errors = self._write_mixdowns(served, custom_output_names, tap1, tap2)
                    for i, names in written.items():
                        if i not in errors:
                            results[i] = results[i] + names
                    for i, e in errors.items():
                        self.logger.error(f"{paths[i]}: {e}")
                        self.batch_errors[i] = e
                if handed:
                    self.last_handoff_gain = handed[-1][3]
        finally:
            first._writer_tap = then._writer_tap = None
            then._injected = None
        self.last_paths_taken = taken
        return results
