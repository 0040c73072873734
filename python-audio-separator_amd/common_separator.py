"""The plugin-surface base class: what ``Separator.load_model`` / ``_separate_file`` expect of a model instance.

Mirror of audio_separator/separator/common_separator.py:CommonSeparator (reference file:line cited per member):
same constructor key set (``common_config`` built at separator.py:867-886), same public attributes the orchestrator
reads and writes (``output_dir`` separator.py:1087-1088, ``is_roformer_model`` / ``get_roformer_loading_stats`` :926-929,
``write_audio`` :1379), same stem naming, same file naming and the same per-file state reset.  The sample
arithmetic of the edges (``spec_utils.normalize``, int16 quantisation, channel interleave) runs in libasx.so through
``self.engine``; decode / encode containers stay on the host (audio_io.py).  There is no CPU path for the arithmetic:
a subclass without an engine cannot write audio.
"""
from __future__ import annotations

import contextlib
import functools
import gc
import logging
import os
import re
import threading

import numpy as np

from . import audio_io


class CommonSeparator:
    # Stem vocabulary (common_separator.py:19-53).  The names are part of the contract: the orchestrator, the ensembler presets
    # and the output file names refer to them.  Kept as one table; the class attributes are generated from it below.
    _STEM_LABELS = {
        "ALL_STEMS": "All Stems", "PRIMARY_STEM": "Primary Stem", "SECONDARY_STEM": "Secondary Stem",
        # instruments, and the name of "everything but" each of them
        "VOCAL_STEM": "Vocals", "INST_STEM": "Instrumental",
        "OTHER_STEM": "Other", "NO_OTHER_STEM": "No Other",
        "BASS_STEM": "Bass", "NO_BASS_STEM": "No Bass",
        "DRUM_STEM": "Drums", "NO_DRUM_STEM": "No Drums",
        "GUITAR_STEM": "Guitar", "NO_GUITAR_STEM": "No Guitar",
        "PIANO_STEM": "Piano", "NO_PIANO_STEM": "No Piano",
        "SYNTH_STEM": "Synthesizer", "NO_SYNTH_STEM": "No Synthesizer",
        "STRINGS_STEM": "Strings", "NO_STRINGS_STEM": "No Strings",
        "WOODWINDS_STEM": "Woodwinds", "NO_WOODWINDS_STEM": "No Woodwinds",
        "BRASS_STEM": "Brass", "NO_BRASS_STEM": "No Brass",
        "WIND_INST_STEM": "Wind Inst", "NO_WIND_INST_STEM": "No Wind Inst",
        "NO_STEM": "No ",
        # karaoke / backing-vocal models
        "LEAD_VOCAL_STEM": "lead_only", "BV_VOCAL_STEM": "backing_only",
        "LEAD_VOCAL_STEM_I": "with_lead_vocals", "BV_VOCAL_STEM_I": "with_backing_vocals",
        "LEAD_VOCAL_STEM_LABEL": "Lead Vocals", "BV_VOCAL_STEM_LABEL": "Backing Vocals",
    }
    locals().update(_STEM_LABELS)

    _CONFIG_KEYS = ("log_level", "torch_device", "torch_device_cpu", "torch_device_mps", "onnx_execution_provider",
                    "model_name", "model_path", "model_data", "output_dir", "output_format", "output_bitrate",
                    "normalization_threshold", "amplification_threshold", "enable_denoise", "output_single_stem",
                    "invert_using_spec", "sample_rate", "use_soundfile")

    def __init_subclass__(cls, **kw):
        """Every architecture's ``separate`` returns only after the container writes it started have finished (the built-in WAV
        writer runs on worker threads so that the files of a song are written concurrently and overlap the next stem's int16
        pass; the orchestrator may open the files as soon as ``separate`` returns)."""
        super().__init_subclass__(**kw)
        inner = cls.__dict__.get("separate")
        if inner is not None:
            @functools.wraps(inner)
            def separate(self, *args, **kwargs):
                with self._writing():
                    return inner(self, *args, **kwargs)
            cls.separate = separate

    def __init__(self, config: dict):
        """common_separator.py:55-148."""
        self.logger = config.get("logger") or logging.getLogger("audio_separator_amd")
        for key in self._CONFIG_KEYS:
            setattr(self, key, config.get(key))
        if self.model_data is None:
            self.model_data = {}
        self.engine = None                       # the libasx.so handle; set by the architecture subclass
        self.asx_profile_file = bool(config.get("asx_profile_file"))   # per-phase wall times of separate() in file_timings
        self.asx_input_resample = self._input_resample_mode(config)    # who converts a file at another rate than the model's
        self.asx_output_encoder = self._output_encoder_mode(config)    # who compresses a .flac stem when pydub is installed
        self.asx_output_rate = self._output_rate_mode(config)          # the rate and frame count stems are written at
        self.asx_complement_rate = self._complement_rate_mode(config, self.asx_output_rate)   # the rate the complement stem is formed at
        self._complement_noted = False           # (the "nothing to do for this model" note: once per instance)
        self.asx_autocast = self._autocast_mode(config)                # whether the Roformer engine runs its single-product kernels
        if self.asx_autocast == "follow" and self._autocast_refusal:
            self.logger.info(f"asx_autocast='follow' does nothing on {type(self).__name__}: {self._autocast_refusal}")
        self.file_timings = {}
        self._pending_writes = []                # (thread, error box) of container writes in flight
        # how the last stem reached its encoder: "flac_device_resident" | "flac_device_upload" (.flac), "wav_device_resident" (a .wav of
        # write_audio_soundfile whose samples were converted to the file's format in HBM)
        self.last_write_path = None

        self.roformer_loader = None
        self.is_roformer_model = self._detect_roformer_model()
        if self.is_roformer_model:
            self._initialize_roformer_loader()

        self.primary_stem_name = None
        self.secondary_stem_name = None
        self.input_bit_depth = None
        self.input_subtype = None

        training = self.model_data.get("training") if isinstance(self.model_data, dict) else None
        instruments = (training or {}).get("instruments") if isinstance(training, dict) else None
        if instruments:
            target = training.get("target_instrument")
            # a target that is listed second names the model's actual output (common_separator.py:112-122)
            if target and len(instruments) >= 2 and instruments[0] != target and instruments[1] == target:
                self.primary_stem_name, self.secondary_stem_name = instruments[1], instruments[0]
            else:
                self.primary_stem_name = instruments[0]
                self.secondary_stem_name = instruments[1] if len(instruments) > 1 else self.secondary_stem(instruments[0])
        if self.primary_stem_name is None:
            self.primary_stem_name = self.model_data.get("primary_stem", "Vocals")
            self.secondary_stem_name = self.secondary_stem(self.primary_stem_name)

        self.is_karaoke = self.model_data.get("is_karaoke", False)
        self.is_bv_model = self.model_data.get("is_bv_model", False)
        self.bv_model_rebalance = self.model_data.get("is_bv_model_rebalanced", 0)

        self.logger.debug(f"Common params: model_name={self.model_name}, model_path={self.model_path}, "
                          f"output_dir={self.output_dir}, output_format={self.output_format}")
        self.logger.debug(f"Common params: primary_stem_name={self.primary_stem_name}, "
                          f"secondary_stem_name={self.secondary_stem_name}")

        self._reset_file_state()
        self.cached_sources_map = {}

    # ``common_config["asx_input_resample"]``: "host" (the default) leaves a file whose rate is not ``sample_rate`` to librosa.load, as the
    # reference does (soxr_hq on one host thread; AudioIOError where librosa is not installed); "device" converts a RIFF/WAVE file with
    # the engine's rational polyphase converter (asx_resample_rational: this project's own filter in soxr_hq's class, so the samples
    # differ from the reference's in the transition band -- hence opt-in).  The environment variable ASX_INPUT_RESAMPLE, when set and
    # not empty, overrides the configuration of every plugin of the process.
    INPUT_RESAMPLE_MODES = ("host", "device")
    _resamples_input_files = True      # (a plugin whose reference loads files through another converter says False)

    @classmethod
    def _input_resample_mode(cls, config) -> str:
        mode = os.environ.get("ASX_INPUT_RESAMPLE") or config.get("asx_input_resample") or "host"
        if mode not in cls.INPUT_RESAMPLE_MODES:
            raise ValueError(f"asx_input_resample must be one of {cls.INPUT_RESAMPLE_MODES}, not {mode!r}")
        return mode

    # ``common_config["asx_output_encoder"]``: who writes a ``.flac`` stem where pydub is installed.  "host" (the default): pydub / ffmpeg, as
    # the reference does; "device": the engine's encoder (asx_flac_encode_dev) and audio_io.write_flac.  Without pydub the built-in encoder
    # writes FLAC under either setting, as the built-in writer does for WAV.  The environment variable ASX_OUTPUT_ENCODER, when set and not
    # empty, overrides the configuration of every plugin of the process.  Other compressed formats always need pydub.
    # With ``use_soundfile`` the same knob decides for soundfile: "host" leaves every stem to sf.write where soundfile is installed; "device"
    # converts a stem that is still in HBM there (asx_pcm_encode_dev / asx_flac_encode_pcm_dev) -- opt-in because libsndfile multiplies in
    # float32 where this project (audio_io.write_wav's rule) multiplies in float64, so single samples can differ by one unit.  Without
    # soundfile the device path is taken under either setting.
    OUTPUT_ENCODER_MODES = ("host", "device")

    @classmethod
    def _output_encoder_mode(cls, config) -> str:
        mode = os.environ.get("ASX_OUTPUT_ENCODER") or config.get("asx_output_encoder") or "host"
        if mode not in cls.OUTPUT_ENCODER_MODES:
            raise ValueError(f"asx_output_encoder must be one of {cls.OUTPUT_ENCODER_MODES}, not {mode!r}")
        return mode

    # ``common_config["asx_output_rate"]``: "model" (the default) writes every stem at ``sample_rate``, as the reference does; "input" writes
    # it at the input file's own sample rate with exactly its frame count: ``write_audio`` converts the stem with the engine's rational
    # polyphase converter (asx_resample_rational_stem: this project's own filter, parity against soxr unpinned -- hence opt-in) before the
    # normalise / quantise pass.  ``primary_source`` / ``secondary_source`` and what ``stems_dev`` returns stay at the model's rate.  There
    # is no environment override: the plugins named below refuse "input", and a process-wide switch would break them.
    OUTPUT_RATE_MODES = ("model", "input")
    _output_rate_refusal = None        # (a plugin that cannot write at the input's rate says why)

    @classmethod
    def _output_rate_mode(cls, config) -> str:
        mode = config.get("asx_output_rate") or "model"
        if mode not in cls.OUTPUT_RATE_MODES:
            raise ValueError(f"asx_output_rate must be one of {cls.OUTPUT_RATE_MODES}, not {mode!r}")
        if mode == "input" and cls._output_rate_refusal:
            raise ValueError(f"asx_output_rate='input' is not supported by {cls.__name__}: {cls._output_rate_refusal}")
        return mode

    # ``common_config["asx_complement_rate"]``: "model" (the default) forms the complement stem -- the MDX secondary ``mix - compensate *
    # primary``, the residual row of a single-target MDXC / Roformer model -- at the model's rate and converts it like every other stem, so
    # with ``asx_output_rate`` = "input" it carries nothing above the converter's pass band.  "input" (needs ``asx_output_rate`` = "input" on
    # the same plugin) forms the complement FILE at the file's rate against the file's own decoded mix, inside the stem converter's pass
    # (asx_resample_rational_complement): c_f = fl(fl(s * mix_f) - fl(k * r)), r the converted model stem, s the factor the mix normalise
    # applied, k ``compensate`` (MDX) or 1 -- the two stems then sum to s * the file.  ``primary_source`` / ``secondary_source``, what
    # ``write_audio`` is handed and ``stems_dev`` stay at the model's rate.  No environment override, as for ``asx_output_rate``.
    COMPLEMENT_RATE_MODES = ("model", "input")
    _complement_rate_refusal = None    # (a plugin none of whose stems is a difference against the mix says why)

    @classmethod
    def _complement_rate_mode(cls, config, output_rate="model") -> str:
        mode = config.get("asx_complement_rate") or "model"
        if mode not in cls.COMPLEMENT_RATE_MODES:
            raise ValueError(f"asx_complement_rate must be one of {cls.COMPLEMENT_RATE_MODES}, not {mode!r}")
        if mode == "input" and cls._complement_rate_refusal:
            raise ValueError(f"asx_complement_rate='input' is not supported by {cls.__name__}: {cls._complement_rate_refusal}")
        if mode == "input" and output_rate != "input":
            raise ValueError("asx_complement_rate='input' requires asx_output_rate='input' on the same plugin: the complement is formed at "
                             "the file's rate only where the stems are written at it")
        return mode

    # ``common_config["asx_autocast"]``: the arithmetic of the Roformer engine's linears and attention.  "off" (the default): the fp32-grade
    # fp16 x 3 kernels, and the engine option is never touched -- also inside an ambient ``torch.autocast`` context.  "fp16": every engine call
    # of the plugin runs the single-product kernels (engine option "gemm_f16x1", include/asx.h: REDUCED PRECISION, opt-in, not the reference's
    # bits; activations, norms, softmax, rotary, STFT / iSTFT stay fp32, which the reference's autocast does not guarantee).  "follow": as
    # "fp16" for a call made while ``torch.is_autocast_enabled("cuda")`` is true and as "off" otherwise -- this is how the orchestrator's
    # ``use_autocast`` (it wraps ``separate`` in ``torch.autocast``) reaches a plugin.  Only the Roformer engine has single-product kernels:
    # the plugins that say so in ``_autocast_refusal`` refuse "fp16" and accept "follow" without effect (one info line), so an orchestrator
    # that passes "follow" to every model keeps working.  The option is per engine and set before every engine call; a captured graph
    # (sharding.ShardWorkspace: its graph keys do not include engine options) keeps the arithmetic it was captured with.  No environment override.
    AUTOCAST_MODES = ("off", "fp16", "follow")
    _autocast_refusal = None           # (a plugin whose engine has no single-product kernels says so)
    _AUTOCAST_ONLY_ROFORMER = "only the Roformer engine has single-product kernels"

    @classmethod
    def _autocast_mode(cls, config) -> str:
        mode = config.get("asx_autocast") or "off"
        if mode not in cls.AUTOCAST_MODES:
            raise ValueError(f"asx_autocast must be one of {cls.AUTOCAST_MODES}, not {mode!r}")
        if mode == "fp16" and cls._autocast_refusal:
            raise ValueError(f"asx_autocast='fp16' is not supported by {cls.__name__}: {cls._autocast_refusal}")
        return mode

    @staticmethod
    def _autocast_active(mode) -> bool:
        """Whether a call made now runs the single-product kernels under ``mode``."""
        if mode == "fp16":
            return True
        if mode == "follow":
            import torch
            return bool(torch.is_autocast_enabled("cuda"))
        return False

    def _complement_stem_name(self):
        """Hook: the name of the stem this plugin forms as ``s * mix - k * (its model stem)`` under the current options, None when it has
        none (the base class, a multi-stem model, a spectral inversion)."""
        return None

    def _keeps_file_mix(self) -> bool:
        """whether the decoded mix of a file that is being converted to the model's rate is kept for the complement's write"""
        if getattr(self, "asx_complement_rate", "model") != "input" or getattr(self, "_stems_only", False):
            return False                   # (``_stems_only``: stems_dev / stems_dev_many write nothing)
        name = self._complement_stem_name()
        return name is not None and self._wanted(name)

    def _note_no_complement(self, why: str):
        if getattr(self, "asx_complement_rate", "model") == "input" and not self._complement_noted:
            self._complement_noted = True
            self.logger.info(f"asx_complement_rate='input' does nothing here: {why}")

    def _normalize_factor(self, peak) -> float:
        """The float32 factor ``Engine.normalize`` with the plugin's thresholds applies to an array of this peak (1.0: none) -- the rule of
        spec_utils.normalize as csrc/kernels_fft.h normalize_kernel restates it."""
        peak, thr, amp = np.float32(peak), np.float32(self.normalization_threshold), self.amplification_threshold
        if peak > thr:
            return float(thr / peak)
        if amp is not None and peak < np.float32(amp):
            return float(np.float32(amp) / peak)
        return 1.0

    def _mix_factor(self, dev_mix, host_mix, kept=None) -> float:
        """``s``: what the in-place normalise of the model-rate mix is about to multiply it by; 1.0 where nobody will ask (no kept mix --
        ``kept`` says so for a file of a pool, the current file's state otherwise)."""
        if not (self._file_mix is not None if kept is None else kept):
            return 1.0
        if dev_mix is not None:
            return self.engine.normalize_scale_dev(dev_mix.data_ptr(), dev_mix.numel(), self.normalization_threshold, self.amplification_threshold,
                                                   stream=self._stream())
        return self._normalize_factor(np.abs(host_mix).max())

    def _register_complement(self, complement_source, model_source, stem_scale: float, normalise: bool, model_wanted: bool = True):
        """The plugin, when it emits a file's stems: ``complement_source`` (the array it hands to write_audio for the complement stem) is
        ``_mix_scale * mix - stem_scale * model_source``; ``normalise``: the per-stem normalise follows (MDXC); ``model_wanted``: the model
        stem is written as well.  Without a kept mix, or when the complement is not written, nothing is registered and the kept mix is
        released."""
        self._complement = None
        if self._file_mix is None:
            # the stems of this file are converted, the complement is wanted, and no decode left the file's own mix behind (a container
            # only librosa reads, a decode that disagrees with the header): said once per file, not passed over in silence
            name = self._complement_stem_name()
            if (getattr(self, "asx_complement_rate", "model") == "input" and complement_source is not None and name is not None
                    and self._wanted(name) and self._output_rate_target() is not None):
                self.logger.warning(f"{self.audio_file_path}: asx_complement_rate='input', but the file's own mix was not kept by its decoder: "
                                    f"the {name} stem is written from the difference at {self.sample_rate} Hz")
            return
        name = self._complement_stem_name()
        if complement_source is None or name is None or not self._wanted(name) or self._output_rate_target() is None:
            self._file_mix = None
            return
        self._complement = {"complement": complement_source, "model": model_source, "k": float(stem_scale), "normalise": bool(normalise),
                            "model_wanted": bool(model_wanted), "complement_wanted": True, "converted": None}

    def _resample_plan(self, file_rate):
        """(n_out for n_in) -> callable when ``asx_input_resample`` is "device" and the engine's converter takes ``file_rate`` ->
        ``sample_rate``; None otherwise (the setting is "host", the rates are equal, the pair is refused: behave as before)."""
        if getattr(self, "asx_input_resample", "host") != "device" or self.engine is None or not self.sample_rate:
            return None
        if not self._resamples_input_files:
            return None
        if file_rate == self.sample_rate or not hasattr(self.engine, "resample_rational_plan"):
            return None
        try:
            self.engine.resample_rational_plan(file_rate, self.sample_rate, 1)
        except Exception as e:
            self.logger.debug(f"no device converter for {file_rate} -> {self.sample_rate} Hz ({e}): the host decoder takes the file")
            return None
        return lambda n_in: self.engine.resample_rational_plan(file_rate, self.sample_rate, n_in)[0]

    # what one input file leaves behind (common_separator.py:136-147, 509-520): reset by clear_file_specific_paths
    _FILE_STATE = ("audio_file_path", "audio_file_base", "primary_source", "secondary_source", "primary_stem_output_path",
                   "secondary_stem_output_path")

    def _reset_file_state(self):
        for name in self._FILE_STATE:
            setattr(self, name, None)
        self._dev_stems = {}          # id(host array) -> (host array, device tensor [N, 2]): stems that never left HBM
        self._file_seconds = None     # duration of the current input, probed once per file
        self._file_rate = self._file_frames = None     # the input's own sample rate and frame count, where its header was read
        self._out_rate_group = None   # asx_output_rate = "input": (planar device stems [S, 2, N], the same at the file's rate)
        self._out_rate_warned = False
        # asx_complement_rate = "input": the file's own decoded mix [2, F] (a CUDA tensor, or a host array on the host route) while the
        # complement is still to be written, the factor the mix normalise applied, and what the plugin registered (_register_complement)
        self._file_mix, self._mix_scale, self._complement = None, 1.0, None
        self.last_arithmetic = None   # "fp16x3" | "fp16x1": what the Roformer engine ran this file's linears and attention on (asx_autocast)

    # ---- steps every architecture's separate() shares ---------------------------------------------------------------
    def _read_options(self, arch_config: dict, table):
        """``table`` = ((key, default), ...): the architecture options the orchestrator passes (separator.py:125-128)."""
        for key, default in table:
            setattr(self, key, arch_config.get(key, default))

    def _keep_configs(self, common_config: dict, arch_config: dict):
        """What ``load_model`` builds the demixer from.  ``asx_max_batch`` is an engine knob, not a reference option: chunks per
        device batch (results do not depend on it)."""
        self._common, self._arch = dict(common_config), dict(arch_config)
        self._max_batch = int(arch_config.get("asx_max_batch", 0))

    def _begin_file(self, audio_file_path: str):
        self.audio_file_path = audio_file_path
        self.audio_file_base = os.path.splitext(os.path.basename(audio_file_path))[0]
        self._dev_stems = {}
        self._file_seconds = None
        self._file_rate = self._file_frames = None
        self._out_rate_group = None
        self._out_rate_warned = False
        self._file_mix, self._mix_scale, self._complement = None, 1.0, None
        self.file_timings = {}        # seconds per phase of this file when ``asx_profile_file`` is set (bench.py file_level)

    # ---- device-resident file path (load / normalise / write edges without host round trips) -----------------
    # ---- concurrent container writes -----------------------------------------------------------------------------
    def _write_wav_async(self, stem_path, pcm, subtype):
        """audio_io.write_wav on a worker thread (the file write releases the GIL); drained before ``separate`` returns."""
        rate = self._container_rate()
        self._write_async(lambda: audio_io.write_wav(stem_path, pcm, rate, subtype))

    def _write_async(self, write):
        """``write()`` -- one container write -- on a worker thread; drained before ``separate`` returns."""
        # a write_audio call from outside separate() (the orchestrator's ensemble output, separator.py:1379) is synchronous:
        # nobody would drain it
        if os.environ.get("ASX_ASYNC_WRITES", "1") == "0" or not getattr(self, "_in_separate", False):
            write()
            return
        box = []

        def work():
            try:
                write()
            except BaseException as e:          # re-raised by _drain_writes on the caller's thread
                box.append(e)
        t = threading.Thread(target=work, name="asx-wav-writer", daemon=True)
        t.start()
        self._pending_writes.append((t, box))

    def _drain_writes(self, raise_errors: bool = True):
        t0 = self._now()
        pending, self._pending_writes = self._pending_writes, []
        err = None
        for t, box in pending:
            t.join()
            if box and err is None:
                err = box[0]
        if pending and getattr(self, "asx_profile_file", False):
            self.file_timings["write_drain"] = self.file_timings.get("write_drain", 0.0) + (self._now() - t0)
        if err is not None:
            if raise_errors:
                raise err
            self.logger.error(f"a container write failed: {err}")

    @contextlib.contextmanager
    def _writing(self):
        """The span in which write_audio may leave container writes to worker threads: they have finished when it ends."""
        self._in_separate = True
        try:
            yield
        except BaseException:
            self._in_separate = False
            self._drain_writes(raise_errors=False)      # the caller's exception wins over a writer's
            raise
        self._in_separate = False
        self._drain_writes()

    def _tick(self, phase: str, t0: float) -> float:
        """Accumulate wall time of ``phase`` since ``t0`` (device drained first) when per-file profiling is on."""
        if not getattr(self, "asx_profile_file", False):
            return t0
        import time
        self._sync()
        t1 = time.perf_counter()
        self.file_timings[phase] = self.file_timings.get(phase, 0.0) + (t1 - t0)
        return t1

    def _now(self) -> float:
        import time
        return time.perf_counter()

    def _torch_device(self):
        import torch
        return torch.device("cuda", self.engine.device)

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self._torch_device()).cuda_stream

    def _sync(self):
        import torch
        if self.engine is not None and torch.cuda.is_available():
            torch.cuda.current_stream(self._torch_device()).synchronize()

    def _fast_file_path_enabled(self) -> bool:
        if self.engine is None or os.environ.get("ASX_FILE_FASTPATH", "1") == "0" or not hasattr(self.engine, "pcm_decode_dev"):
            return False
        try:
            import torch
            return torch.cuda.is_available()      # torch is the allocator of the pinned / device staging buffers
        except Exception:
            return False

    # ---- the door for a caller that already holds a file's mix in HBM (workflow.ChainSeparator) ------------------------------------------
    # ``_inject_mix(path, mix, state, peak)`` makes the next ``_device_mix(path)`` -- which ``_load_mix`` / ``_device_decode`` and the
    # MDXC plugin's own calls all end in -- return ``mix`` (CUDA tensor [2, N] at ``sample_rate``) and record ``state`` (the per-file
    # attributes a decode of that file would have left) instead of opening the path; ``peak`` (max |mix|) feeds the silent-file refusal.
    # An injection is used once.  Without one nothing here does anything.
    _injected = None
    # a listener on ``final_process`` and the device writers, set by the same caller for the span of a call: see ``_tap_stem``
    _writer_tap = None

    def _inject_mix(self, path, mix, state, peak):
        if self._injected is None:
            self._injected = {}
        self._injected[path] = (mix, dict(state), float(peak))

    def _injected_for(self, path):
        return self._injected.get(path) if self._injected and isinstance(path, str) else None

    def _takes_device_mix(self) -> bool:
        """Hook: whether ``_device_decode`` hands a device-resident mix on at all (a plugin that sends some models to the host says no)."""
        return True

    def _take_injected(self, path, check_silent):
        mix, state, peak = self._injected.pop(path)
        for key, value in state.items():
            setattr(self, key, value)
        if check_silent and not peak > 0.0:
            msg = f"Audio file {path} is empty or not valid"
            self.logger.error(msg)
            raise ValueError(msg)
        return mix

    def _tap_stem(self, dev_stem, layout, n, encoded, subtype, peak):
        """The device writers, once per stem they take from HBM: the float stem (not normalised), the buffer its samples were encoded
        into on the device (None where the hand-off has no use for it: the int32 containers of a soundfile FLAC) with the WAV subtype a
        reader would decode it as, and the peak after normalisation."""
        tap = self._writer_tap
        if tap is not None:
            tap.encoded(self, dev_stem, layout, n, encoded, subtype, peak)

    def _device_mix(self, path, check_silent=True):
        """prepare_mix for a RIFF/WAVE file at the model's rate WITHOUT a host float array: the data chunk is read into pinned
        memory, copied to HBM once and converted to the planar float32 mix [2, N] on the device (asx_pcm_decode_dev: the same
        x / 2^(bits-1) conversion libsndfile applies under librosa.load, common_separator.py:252).  With ``asx_input_resample`` =
        "device" a file at another rate is decoded at its own frame count and brought to ``sample_rate`` by
        asx_resample_rational_dev ([2, ceil(N * sample_rate / file rate)]).  A native FLAC file takes ``_device_mix_flac``.  Returns a CUDA tensor, or
        None when the file needs the host decoder (other container, other rate, exotic subtype) -- the caller then takes
        prepare_mix.  Raises the reference's ValueError for a silent file (:268-271) unless ``check_silent`` is False: the VR
        plugin never calls prepare_mix (vr_separator.py:255-291 loads with librosa directly), so a silent file must come out the
        same whichever decode path it took (the writer's "nothing to write" branch handles silent stems)."""
        if self._injected_for(path) is not None:
            return self._take_injected(path, check_silent)
        if not self._fast_file_path_enabled() or not isinstance(path, str):
            return None
        import torch
        try:
            info = audio_io.wav_info(path)
        except (audio_io.AudioIOError, OSError):
            return self._device_mix_flac(path, check_silent) if audio_io.is_flac(path) else None
        if info["subtype"] not in self.engine.PCM_FORMATS or info["frames"] < 1 or info["channels"] > 2:
            return None                # (more than two channels: prepare_mix + the reference's "Expected a 2-channel" error)
        n_resampled = None             # a file at another rate: only with asx_input_resample = "device" and a pair the converter takes
        if info["samplerate"] != self.sample_rate:
            n_resampled = self._resample_plan(info["samplerate"])
            if n_resampled is None:
                return None
        t0 = self._now()
        # what _probe_bit_depth records for the writer (common_separator.py:231-250)
        self.input_subtype = st = info["subtype"]
        self.input_bit_depth = 16 if st == "PCM_16" else (24 if st == "PCM_24" else 32)
        self._file_seconds = info["frames"] / float(info["samplerate"])
        self._file_rate, self._file_frames = info["samplerate"], info["frames"]
        frames, ch = info["frames"], info["channels"]
        nbytes = frames * ch * info["bits"] // 8
        staged = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        with open(path, "rb") as f:
            f.seek(info["data_offset"])
            got = f.readinto(memoryview(staged.numpy()))
        if got != nbytes:
            return None
        t0 = self._tick("read", t0)
        dev = self._torch_device()
        raw = staged.to(dev, non_blocking=True)
        mix = torch.empty((2, frames), dtype=torch.float32, device=dev)
        peak = self.engine.pcm_decode_dev(raw.data_ptr(), frames, ch, st, mix.data_ptr(), stream=self._stream())
        t0 = self._tick("h2d_decode", t0)
        if check_silent and not peak > 0.0:
            msg = f"Audio file {path} is empty or not valid"
            self.logger.error(msg)
            raise ValueError(msg)
        if n_resampled is not None:
            n_out = n_resampled(frames)
            at_rate = torch.empty((2, n_out), dtype=torch.float32, device=dev)
            self.engine.resample_rational_dev(mix.data_ptr(), 2, frames, info["samplerate"], self.sample_rate, at_rate.data_ptr(), n_out,
                                              stream=self._stream())
            if self._keeps_file_mix():
                self._file_mix = mix       # 8 * frames bytes of HBM, until the complement stem is written
            mix = at_rate
            self._tick("resample", t0)
        return mix

    def _device_mix_flac(self, path, check_silent=True):
        """``_device_mix`` for a native FLAC file (found by its marker) of 16 or 24 bits and at most two channels: the audio frames are
        read into pinned memory, copied to HBM once and decoded there (Engine.flac_decode_scan_dev / flac_decode_finish_dev) into the
        mix libsndfile gives, x / 2^(bits-1).  None for every other stream, a file at another rate without a device converter, or an
        engine without the decoder."""
        if not hasattr(self.engine, "flac_decode_scan_dev"):
            return None
        import torch
        try:
            info = audio_io.flac_stream(path)
            self.engine.flac_decode_plan(info["audio_bytes"], info["channels"], info["bits_per_sample"], info["max_blocksize"], info["max_framesize"])
        except Exception as e:
            self.logger.debug(f"{path}: no device FLAC decode ({e})")
            return None
        if info["bits_per_sample"] not in (16, 24) or info["channels"] > 2:
            return None
        n_resampled = None
        if info["samplerate"] != self.sample_rate:
            n_resampled = self._resample_plan(info["samplerate"])
            if n_resampled is None:
                return None
        t0 = self._now()
        nbytes = info["audio_bytes"]
        staged = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        with open(path, "rb") as f:
            f.seek(info["audio_offset"])
            got = f.readinto(memoryview(staged.numpy()))
        if got != nbytes:
            return None
        t0 = self._tick("read", t0)
        dev = self._torch_device()
        raw = staged.to(dev, non_blocking=True)
        found = self.engine.flac_decode_scan_dev(raw.data_ptr(), nbytes, info, stream=self._stream())
        frames = found["n_samples"]
        if found["bytes_consumed"] < nbytes:
            self.logger.warning(f"{path}: FLAC frames end at byte {found['bytes_consumed']} of {nbytes} of the audio part (a trailing tag, a cut "
                                f"file or a damaged frame); the {found['n_frames']} frames before it are used")
        if frames < 1:
            msg = f"Audio file {path} is empty or not valid"
            self.logger.error(msg)
            raise ValueError(msg)
        # what _probe_bit_depth records for the writer (common_separator.py:231-250)
        self.input_subtype = "PCM_16" if info["bits_per_sample"] == 16 else "PCM_24"
        self.input_bit_depth = info["bits_per_sample"]
        self._file_seconds = frames / float(info["samplerate"])
        self._file_rate, self._file_frames = info["samplerate"], frames      # (the scanned count: STREAMINFO's is a hint)
        mix = torch.empty((2, frames), dtype=torch.float32, device=dev)
        peak = self.engine.flac_decode_finish_dev(mix.data_ptr(), frames, stream=self._stream())
        t0 = self._tick("flac_decode", t0)
        if check_silent and not peak > 0.0:
            msg = f"Audio file {path} is empty or not valid"
            self.logger.error(msg)
            raise ValueError(msg)
        if n_resampled is not None:
            n_out = n_resampled(frames)
            at_rate = torch.empty((2, n_out), dtype=torch.float32, device=dev)
            self.engine.resample_rational_dev(mix.data_ptr(), 2, frames, info["samplerate"], self.sample_rate, at_rate.data_ptr(), n_out,
                                              stream=self._stream())
            if self._keeps_file_mix():
                self._file_mix = mix       # 8 * frames bytes of HBM, until the complement stem is written
            mix = at_rate
            self._tick("resample", t0)
        return mix

    def _device_decode(self, path):
        """``_device_mix`` where the plugin lets the device decoder have the file (hook)."""
        return self._device_mix(path)

    def _require_stereo(self, mix):
        """The plugin's own refusal of a host mix that is not [2, N] (hook: the texts differ between the architectures)."""

    def _host_mix(self, path):
        mix = self.prepare_mix(path)
        self._require_stereo(mix)
        return np.ascontiguousarray(mix, np.float32)

    def _load_mix(self, path):
        """One input file as a mix [2, N]: (CUDA tensor, None) when the device decoder takes it, else (None, float32 array) from
        ``prepare_mix``, with the refusals of both."""
        mix = self._device_decode(path)
        return (mix, None) if mix is not None else (None, self._host_mix(path))

    def _device_mixes(self, mixes):
        """What ``_load_mix`` returned for a list of files -> all of them on the device."""
        import torch
        dev = self._torch_device()
        return [d if d is not None else torch.from_numpy(h).to(dev) for d, h in mixes]

    @staticmethod
    def _to_host(stems):
        return stems if isinstance(stems, np.ndarray) else stems.cpu().numpy()

    def _host_stem(self, dev_stem):
        """A device stem [N, 2] as the numpy array the reference leaves in ``primary_source`` / ``secondary_source`` (pinned
        staging, one asynchronous copy) and remember which device tensor it mirrors, so write_audio can quantise on the device
        instead of uploading the array again."""
        import torch
        host = torch.empty(dev_stem.shape, dtype=dev_stem.dtype, pin_memory=True)
        host.copy_(dev_stem, non_blocking=True)
        arr = host.numpy()
        # the mirror is READ-ONLY: write_audio quantises from the device tensor, so an in-place edit of the host array between
        # separate() and write_audio would be silently dropped -- it raises instead (assign a NEW array to take the generic path)
        arr.flags.writeable = False
        self._dev_stems[id(arr)] = (arr, dev_stem, host, "rows")
        return arr

    def _host_planar_stems(self, dev_stems):
        """Device stems [S, 2, N] -> their pinned host mirror [S, 2, N] plus the [N, 2] VIEWS (``source[i].T``) the reference hands to
        write_audio, each registered against its planar device tensor (the Demucs / MDXC layouts)."""
        import torch
        host = torch.empty(dev_stems.shape, dtype=dev_stems.dtype, pin_memory=True)
        host.copy_(dev_stems, non_blocking=True)
        arr = host.numpy()
        arr.flags.writeable = False        # as in _host_stem: the views below inherit it
        views = []
        for i in range(arr.shape[0]):
            v = arr[i].T
            self._dev_stems[id(v)] = (v, dev_stems[i], host, "planar", (dev_stems, i))
            views.append(v)
        return arr, views

    def _device_stem_entry(self, stem_source):
        hit = self._dev_stems.get(id(stem_source))
        return hit if hit is not None and hit[0] is stem_source else None

    def _device_stem_for(self, stem_source):
        hit = self._device_stem_entry(stem_source)
        return hit[1] if hit is not None else None

    def _wanted(self, stem_name: str) -> bool:
        """``output_single_stem`` filter (mdx_separator.py:185,193)."""
        return not self.output_single_stem or self.output_single_stem.lower() == stem_name.lower()

    def _emit_stem(self, stem_name: str, source, custom_output_names, files: list) -> str:
        path = self.get_stem_output_path(stem_name, custom_output_names)
        self.logger.info(f"{stem_name} -> {path}")
        self.final_process(path, source, stem_name)
        files.append(path)
        return path

    def _wanted_pair(self) -> list:
        """[(stem name, "secondary" | "primary")] of the stems that get written: the secondary one first, then the primary one --
        the order the reference returns them in (mdx_separator.py:184-203)."""
        return [(name, which) for name, which in ((self.secondary_stem_name, "secondary"), (self.primary_stem_name, "primary"))
                if self._wanted(name)]

    def _emit_pair(self, custom_output_names) -> list:
        """``secondary_source`` / ``primary_source`` -> files, as ``_wanted_pair`` orders and filters them."""
        files = []
        for name, which in self._wanted_pair():
            path = self._emit_stem(name, getattr(self, f"{which}_source"), custom_output_names, files)
            setattr(self, f"{which}_stem_output_path", path)
        return files

    # ---- a batch of files in one pooled engine call -----------------------------------------------------------------
    # A plugin that implements the hooks ``_pooled_stems`` and ``_emit_file`` (and ``_prepare_model`` / ``_check_loaded`` where it needs
    # one) publishes the shell as ``separate_many``; the others have no such attribute.  With the hook ``_stems_of`` it also publishes
    # ``_stems_dev_many`` as ``stems_dev_many``: the same pool, the stems left on the device instead of written (ensemble.py).  ``_PER_FILE`` lists what loading a file leaves
    # for its writer; a plugin that records more extends it.
    _PER_FILE = ("audio_file_path", "audio_file_base", "input_bit_depth", "input_subtype", "_file_seconds", "_file_rate", "_file_frames",
                 "_file_mix", "_mix_scale")

    def _prepare_model(self):
        """Hook: what has to be ready before the first file is loaded."""

    def _check_loaded(self, dev_mix, host_mix):
        """Hook: refuse (raise for) a loaded file that the pooled call could not take, so that it fails alone."""

    def _stems_of(self, file_stems):
        """Hook: one entry of ``_pooled_stems`` for a file decoded on the device -> what ``stems_dev`` returns for that file,
        [(stem name, CUDA tensor, "rows" | "planar")] (None: the stems did not stay on the device)."""
        raise NotImplementedError

    def _pool_files(self, paths, device_only=False):
        """The part ``_separate_many`` and ``_stems_dev_many`` share: every file is loaded as ``separate`` loads it (``_load_mix``)
        and checked (``_check_loaded``), then ONE ``_pooled_stems([(device mix or None, host mix or None)])`` call returns the stems
        of all of them.  A file that cannot be used fails alone: the exception is logged and kept in ``self.batch_errors[index]``.
        ``device_only``: a file the device decoder does not take is left out of the pool (and not checked).  Returns
        ([(index, per-file state, device mix, stems)] of the pooled files, [indices left out])."""
        self.batch_errors = {}
        self._prepare_model()
        loaded, left_out = [], []                     # (index, per-file state, device mix, host mix)
        for i, path in enumerate(paths):
            try:
                self._reset_file_state()
                self._begin_file(path)
                dev_mix, host_mix = self._load_mix(path)
                if device_only and dev_mix is None:
                    left_out.append(i)
                    continue
                self._check_loaded(dev_mix, host_mix)
            except Exception as e:
                self._file_failed(i, path, e)
                continue
            loaded.append((i, {k: getattr(self, k) for k in self._PER_FILE}, dev_mix, host_mix))
        if not loaded:
            self._reset_file_state()
            return [], left_out
        self._pool_mix_scales = None                  # (a plugin with a complement stem leaves one factor per loaded file here)
        self._pool_kept = [state["_file_mix"] is not None for _, state, _, _ in loaded]
        stems = self._pooled_stems([(d, h) for _, _, d, h in loaded])
        if self._pool_mix_scales is not None:
            for (_, state, _, _), scale in zip(loaded, self._pool_mix_scales):
                state["_mix_scale"] = scale
            self._pool_mix_scales = None
        if getattr(self, "_pool_arithmetic", None) is not None:       # (a plugin that records the arithmetic of its pooled call: one per call)
            for _, state, _, _ in loaded:
                state["last_arithmetic"] = self._pool_arithmetic
            self._pool_arithmetic = None
        return [(i, state, dev_mix, file_stems) for (i, state, dev_mix, _), file_stems in zip(loaded, stems)], left_out

    def _file_failed(self, i, path, e):                # this file only
        self.logger.error(f"{path}: {e}")
        self.batch_errors[i] = e

    def _restore_file(self, state):
        self._reset_file_state()
        for k, v in state.items():
            setattr(self, k, v)
        if state.get("_file_mix") is not None:
            state["_file_mix"] = None                 # the plugin holds the kept mix now, and releases it when the complement is written

    def _separate_many(self, paths, custom_output_names=None):
        """``separate`` for a list of files with ONE pooled engine call: every file is loaded as ``separate`` loads it
        (``_load_mix``), ``_pooled_stems([(device mix or None, host mix or None)])`` returns the stems of all of them, then
        ``_emit_file(stems, decoded on the device?, custom_output_names)`` -- the step ``separate`` ends with -- writes each file's.
        Returns one list of output names per input, in order; the files are byte-identical to those of ``separate(path)`` called
        per path.

        A file that cannot be used (unreadable, empty or silent, not stereo) fails alone, like the orchestrator's per-file
        ``try``: its entry in the result is an empty list, the exception is logged and kept in ``self.batch_errors[index]``;
        the other files are processed.  ``custom_output_names`` applies to every file, as it does in ``separate``."""
        paths = list(paths)
        results = [[] for _ in paths]
        with self._writing():
            pooled, _ = self._pool_files(paths)
            for i, state, dev_mix, file_stems in pooled:
                self._restore_file(state)
                try:
                    results[i] = self._emit_file(file_stems, dev_mix is not None, custom_output_names)
                except Exception as e:
                    self._file_failed(i, state["audio_file_path"], e)
        return results

    def _stems_dev_many(self, paths):
        """``stems_dev`` for a list of files with ONE pooled engine call (the loading loop and the fail-alone rule of
        ``_separate_many``; nothing is written).  Returns ``(stems, states)``, one entry per input, in order.  ``stems[i]`` is

        * what ``stems_dev(paths[i])`` returns -- [(stem name, CUDA tensor, "rows" | "planar")], honouring ``output_single_stem``;
          the pooled engine calls give every song the bits of the single-song call, so the tensors equal those of ``stems_dev``;
        * None when the file needs the host decoder (it never enters the pool);
        * the exception the file raised (also kept in ``self.batch_errors[i]``).

        ``states[i]`` is the ``_PER_FILE`` state the file left (None unless ``stems[i]`` is a list): restored on the plugin
        (``_restore_file``) it makes ``get_stem_output_path`` name that file's stems.  The plugin's own per-file state is reset
        when the call returns.

        The files are seen in list order, so state that evolves from file to file evolves as in a loop of ``stems_dev``: the
        MDXC short-file rule (at most two pools), the Demucs shift offsets (drawn from ``random`` in file order)."""
        paths = list(paths)
        stems, states = [None] * len(paths), [None] * len(paths)
        self._stems_only = True                       # nothing is written: no file-rate mix is kept, no peak is read back
        try:
            pooled, _ = self._pool_files(paths, device_only=True)
        finally:
            self._stems_only = False
        for i, state, _, file_stems in pooled:
            self._restore_file(state)
            try:
                stems[i] = self._stems_of(file_stems)
                states[i] = state if stems[i] is not None else None
            except Exception as e:
                self._file_failed(i, state["audio_file_path"], e)
        for i, e in self.batch_errors.items():
            stems[i] = e
        self._reset_file_state()
        return stems, states

    # ---- stem naming -------------------------------------------------------
    def secondary_stem(self, primary_stem: str):
        """common_separator.py:150-159."""
        primary_stem = primary_stem if primary_stem else self.NO_STEM
        if primary_stem in self.STEM_PAIR_MAPPER:
            return self.STEM_PAIR_MAPPER[primary_stem]
        if self.NO_STEM in primary_stem:
            return primary_stem.replace(self.NO_STEM, "")
        return f"{self.NO_STEM}{primary_stem}"

    def separate(self, audio_file_path, custom_output_names=None):
        raise NotImplementedError("This method should be overridden by subclasses.")

    def final_process(self, stem_path, source, stem_name):
        """common_separator.py:167-174."""
        self.logger.debug(f"{stem_name}: writing {stem_path}")
        tap = self._writer_tap
        if tap is None:
            self.write_audio(stem_path, source)
            return {stem_name: source}
        tap.begin_stem(self, stem_name, stem_path, source)
        try:
            self.write_audio(stem_path, source)
        finally:
            tap.end_stem(self)
        return {stem_name: source}

    # ---- source cache (common_separator.py:176-215) -----------------------
    def cached_sources_clear(self):
        self.cached_sources_map = {}

    def cached_source_callback(self, model_architecture, model_name=None):
        model, sources = None, None
        for key, value in self.cached_sources_map[model_architecture].items():
            if model_name in key:
                model, sources = key, value
        return model, sources

    def cached_model_source_holder(self, model_architecture, sources, model_name=None):
        self.cached_sources_map[model_architecture] = {**self.cached_sources_map.get(model_architecture, {}),
                                                       **{model_name: sources}}

    # ---- decode edge -------------------------------------------------------
    def _probe_bit_depth(self, path):
        """common_separator.py:231-250: remember the input's sample format so the writer can keep it."""
        try:
            self.input_subtype = audio_io.info(path)["subtype"]
            st = self.input_subtype
            if "PCM_16" in st or st == "PCM_S8":
                self.input_bit_depth = 16
            elif "PCM_24" in st:
                self.input_bit_depth = 24
            elif "PCM_32" in st or "FLOAT" in st or "DOUBLE" in st:
                self.input_bit_depth = 32
            else:
                self.input_bit_depth = 16
                self.logger.warning(f"Unknown audio subtype {st}, defaulting to 16-bit output")
            self.logger.info(f"Input audio subtype: {st}, bit depth: {self.input_bit_depth}")
        except Exception as e:   # the reference swallows every failure here too
            self.logger.warning(f"no container info for {path} ({e}): stems will be written as 16-bit PCM")
            self.input_bit_depth, self.input_subtype = 16, "PCM_16"

    def _probe_file_rate(self, path):
        """``_file_rate`` / ``_file_frames`` of a file the host decodes, from its own header (RIFF/WAVE, or a native FLAC stream whose
        STREAMINFO states its length); another container leaves them unknown."""
        self._file_rate = self._file_frames = None
        if not isinstance(path, str):
            return
        try:
            info = audio_io.wav_info(path)
            self._file_rate, self._file_frames = info["samplerate"], info["frames"]
        except (audio_io.AudioIOError, OSError):
            try:
                info = audio_io.flac_stream(path) if audio_io.is_flac(path) else None
            except (audio_io.AudioIOError, OSError):
                info = None
            if info and info["total_samples"] > 0:
                self._file_rate, self._file_frames = info["samplerate"], info["total_samples"]

    def _load_resampled(self, path):
        """The host-array form of ``_device_mix``'s conversion, for a file the device decoder does not get (ASX_FILE_FASTPATH=0, a plugin
        option that keeps the arrays on the host): audio_io.read_wav, then Engine.resample_rational -- the bits ``_device_mix`` produces.
        None unless ``asx_input_resample`` is "device" and the file is RIFF/WAVE at a rate the converter takes."""
        if getattr(self, "asx_input_resample", "host") != "device" or self.engine is None or not isinstance(path, str):
            return None
        try:
            info = audio_io.wav_info(path)
        except (audio_io.AudioIOError, OSError):
            return None
        if info["frames"] < 1 or self._resample_plan(info["samplerate"]) is None:
            return None
        t0 = self._now()
        x, file_rate = audio_io.read_wav(path)
        t0 = self._tick("read", t0)
        y = self.engine.resample_rational(x, file_rate, self.sample_rate)
        self._tick("resample", t0)
        if self._keeps_file_mix():         # (a mono file is duplicated, as the decoder on the device does)
            self._file_mix = np.ascontiguousarray(np.broadcast_to(x, (2, x.shape[1])) if x.shape[0] == 1 else x[:2], np.float32)
        return (y[0] if y.shape[0] == 1 else y), self.sample_rate

    def _keep_host_decoded_mix(self, path):
        """``asx_complement_rate`` = "input" for a file that the host decoder brought to the model's rate (``asx_input_resample`` = "host",
        a FLAC file without the device file path): its stems are converted back all the same (``_probe_file_rate`` read the header), so the
        file is decoded once more at its own rate and kept.  The complement's algebra does not ask how the model-rate mix was made.  A
        decode that does not give the header's rate and frame count keeps nothing; ``_register_complement`` then says so."""
        if not self._keeps_file_mix() or not self._file_rate or not self._file_frames or self._file_rate == self.sample_rate:
            return
        try:
            x, rate = audio_io.load(path, mono=False, sr=None)
        except Exception as e:
            self.logger.debug(f"{path}: no decode at the file's own rate ({e})")
            return
        x = np.asarray(x, np.float32)
        x = x[None] if x.ndim == 1 else x
        if rate != self._file_rate or x.shape[1] != self._file_frames or x.shape[0] > 2:
            self.logger.debug(f"{path}: decoded as {x.shape} at {rate} Hz, the header says {self._file_frames} frames at {self._file_rate} Hz")
            return
        self._file_mix = np.ascontiguousarray(np.broadcast_to(x, (2, x.shape[1])) if x.shape[0] == 1 else x, np.float32)

    def prepare_mix(self, mix):
        """common_separator.py:217-282: path -> float32 [2, N] at ``sample_rate``; an ndarray [N, ch] is transposed;
        mono is duplicated; an all-zero file raises ValueError."""
        audio_path = mix
        if not isinstance(mix, np.ndarray):
            self._probe_bit_depth(mix)
            self._probe_file_rate(mix)
            got = self._load_resampled(mix)
            if got is None:
                got = audio_io.load(mix, mono=False, sr=self.sample_rate)
                self._keep_host_decoded_mix(audio_path)
            mix, sr = got
            self.logger.debug(f"decoded {audio_path}: {mix.shape[-1]} samples x {mix.shape[0] if mix.ndim > 1 else 1} channel(s) at {sr} Hz")
        else:
            if self.input_bit_depth is None:
                self.input_bit_depth, self.input_subtype = 16, "PCM_16"
            mix = mix.T
        if isinstance(audio_path, str) and not np.any(mix):
            msg = f"Audio file {audio_path} is empty or not valid"
            self.logger.error(msg)
            raise ValueError(msg)
        if mix.ndim == 1:
            mix = np.asfortranarray([mix, mix])
        return mix

    # ---- encode edge -------------------------------------------------------
    def _require_engine(self):
        if self.engine is None:
            raise RuntimeError("no libasx.so engine bound to this separator: the writer's normalise / quantise runs on the "
                               "GPU and has no CPU path")
        return self.engine

    def write_audio(self, stem_path: str, stem_source):
        """common_separator.py:284-303."""
        if self.audio_file_path:
            if self._file_seconds is None:           # probed once per input, not once per stem
                self._file_seconds = audio_io.duration(self.audio_file_path)
            secs = self._file_seconds
            self.logger.info(f"Audio duration is {secs / 3600:.2f} hours ({secs:.2f} seconds).")
        self._write_rate, stem_source = self._at_output_rate(stem_path, stem_source)
        try:
            if self.use_soundfile:
                self.write_audio_soundfile(stem_path, stem_source)
            else:
                self.write_audio_pydub(stem_path, stem_source)
        finally:
            self._write_rate = None

    _write_rate = None       # the rate of the stem write_audio is writing, when it is not ``sample_rate``
    _output_rate_override = None   # (file rate, file frames) for the write_audio call in progress: see _output_rate_target

    def _container_rate(self) -> int:
        return self._write_rate or self.sample_rate

    def _output_rate_target(self):
        """(file rate, file frames) when ``asx_output_rate`` = "input" has this file's stems converted; None when they are written as
        they are: the knob is off, the file is at the model's rate, or -- with one warning per file -- its rate is unknown or the
        converter refuses the pair.  ``_output_rate_override`` = (rate, frames), set around one ``write_audio`` call by a caller that writes
        through this plugin (EnsembleSeparator's ``output_rate`` = "input"), stands for the knob and the file's header for that call."""
        override = self._output_rate_override
        if (override is None and getattr(self, "asx_output_rate", "model") != "input") or self.engine is None or not self.sample_rate:
            return None
        rate, frames = override if override is not None else (self._file_rate, self._file_frames)
        if rate == self.sample_rate:
            return None
        why = None
        if not rate or not frames:
            why = "its own sample rate is unknown (no RIFF/WAVE or FLAC header was read)"
        else:
            try:
                self.engine.resample_rational_plan(self.sample_rate, rate, 1)
            except Exception as e:
                why = f"no converter for {self.sample_rate} -> {rate} Hz ({e})"
        if why is None:
            return rate, frames
        if not self._out_rate_warned:
            self._out_rate_warned = True
            knob = "asx_output_rate='input'" if override is None else "output_rate='input'"
            self.logger.warning(f"{self.audio_file_path}: {knob}, but {why}: the stems are written at {self.sample_rate} Hz")
        return None

    def _soundfile_on_device(self, stem_path: str) -> bool:
        """whether ``_write_soundfile_device`` takes a stem of this name that is still in HBM"""
        sf = audio_io._optional("soundfile")
        if sf is not None and hasattr(sf, "write") and getattr(self, "asx_output_encoder", "host") != "device":
            return False
        return stem_path.lower().split(".")[-1] in ("wav", "flac") and self._output_subtype() in self._DEVICE_WAV_SUBTYPES

    def _at_output_rate(self, stem_path: str, stem_source):
        """``asx_output_rate`` = "input": the stem [n, 2] at ``sample_rate`` -> (file rate, the stem at the file's rate), n_out =
        min(file frames, ceil(n * file rate / sample_rate)) frames -- a full-length stem gets exactly the file's frame count, a shorter
        one (MDX ``invert_using_spec``) its share.  A stem that is still in HBM, and that its writer takes from there, is converted there
        (rows or planar; the planar stems of one file in ONE launch at the first of them) and handed on as a device entry under a
        zero-stride stand-in of the new shape; any other goes through Engine.resample_rational_stem.  (``sample_rate``, the stem itself)
        when nothing is converted.  The two stems ``_register_complement`` named (``asx_complement_rate`` = "input") take
        ``_pair_at_output_rate`` instead."""
        target = self._output_rate_target()
        if target is None:
            return self.sample_rate, stem_source
        a = np.asarray(stem_source)
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0 or a.dtype == np.int16:
            return self.sample_rate, stem_source
        rate, frames = target
        n = a.shape[0]
        n_out = min(int(frames), -(-n * int(rate) // int(self.sample_rate)))
        t0 = self._now()
        entry = self._device_stem_entry(stem_source)
        on_device = entry is not None and (self._soundfile_on_device(stem_path) if self.use_soundfile else True)
        pair = self._complement
        role = None if pair is None else ("complement" if stem_source is pair["complement"] else "model" if stem_source is pair["model"] else None)
        if role is not None:
            out = self._pair_at_output_rate(stem_path, stem_source, role, n, n_out, rate)
        elif on_device:
            import torch
            dev_stem = entry[1]
            group, index = entry[4] if len(entry) > 4 else (None, 0)
            if group is not None and group.is_contiguous():
                if self._out_rate_group is None or self._out_rate_group[0] is not group:
                    y = torch.empty((group.shape[0], 2, n_out), dtype=torch.float32, device=group.device)
                    self.engine.resample_rational_stem_dev(group.data_ptr(), "planar", 2 * group.shape[0], n, self.sample_rate, rate, y.data_ptr(),
                                                           n_out, stream=self._stream())
                    self._out_rate_group = (group, y)
                converted = self._out_rate_group[1][index]
            else:
                dev_stem = dev_stem.contiguous()
                converted = torch.empty((2, n_out), dtype=torch.float32, device=dev_stem.device)
                self.engine.resample_rational_stem_dev(dev_stem.data_ptr(), entry[3], 2, n, self.sample_rate, rate, converted.data_ptr(), n_out,
                                                       stream=self._stream())
            out = np.broadcast_to(np.float32(0), (n_out, 2))      # stands for the shape only: the writers read the device tensor
            self._dev_stems.pop(id(stem_source), None)
            if group is not None and not any(len(e) > 4 and e[4][0] is group for e in self._dev_stems.values()):
                self._out_rate_group = None                        # (the file's last stem: the view keeps the storage until it is written)
            self._dev_stems[id(out)] = (out, converted, None, "planar")
        else:
            if entry is not None:
                self._sync()                                       # (the pinned mirror is filled by an asynchronous copy)
                self._dev_stems.pop(id(stem_source), None)
            out = self.engine.resample_rational_stem(np.ascontiguousarray(a, np.float32), self.sample_rate, rate, n_out, layout="rows").T
        if getattr(self, "asx_profile_file", False):
            self._sync()
        self.file_timings["resample_out"] = self.file_timings.get("resample_out", 0.0) + (self._now() - t0)
        return rate, out

    def _pair_at_output_rate(self, stem_path, stem_source, role, n, n_out, rate):
        """``_at_output_rate`` for the two stems ``_register_complement`` named, ``asx_complement_rate`` = "input": ONE fused launch
        (asx_resample_rational_complement) at whichever of them is written first converts the model stem -- the bits of the plain
        conversion -- and forms the complement against the kept file-rate mix; the other one's tensor (or array) waits in the registration
        for its own write, so neither the model stem's device tensor nor the kept mix has to outlive this call."""
        pair = self._complement
        other = "model" if role == "complement" else "complement"
        if pair["converted"] is not None:                      # the second of the two: converted at the first
            where, kept = pair["converted"]
            self._complement = None
            self._dev_stems.pop(id(stem_source), None)
        else:
            eng = self.engine
            thr, amp = self.normalization_threshold, self.amplification_threshold
            model_entry = self._device_stem_entry(pair["model"])
            mix, self._file_mix = self._file_mix, None          # released with this call
            takes_device = self._soundfile_on_device(stem_path) if self.use_soundfile else True
            other_wanted = pair[f"{other}_wanted"]
            want_y = role == "model" or other_wanted
            if model_entry is not None and takes_device:
                import torch
                where = "device"
                x = model_entry[1].contiguous()
                if isinstance(mix, np.ndarray):
                    mix = torch.from_numpy(mix).to(x.device)
                y = torch.empty((2, n_out), dtype=torch.float32, device=x.device) if want_y else None
                c = torch.empty((2, n_out), dtype=torch.float32, device=x.device)
                eng.resample_rational_complement_dev(x.data_ptr(), model_entry[3], 2, n, self.sample_rate, rate, mix.data_ptr(), mix.shape[1],
                                                     self._mix_scale, pair["k"], y.data_ptr() if want_y else 0, c.data_ptr(), n_out,
                                                     stream=self._stream())
                if pair["normalise"]:
                    eng.normalize_dev(c.data_ptr(), 2 * n_out, thr, amp, stream=self._stream())
            else:
                where = "host"
                if self._device_stem_entry(pair["model"]) is not None or self._device_stem_entry(pair["complement"]) is not None:
                    self._sync()                                # (the pinned mirrors are filled by asynchronous copies)
                if not isinstance(mix, np.ndarray):
                    mix = mix.cpu().numpy()
                y, c = eng.resample_rational_complement(np.ascontiguousarray(np.asarray(pair["model"]), np.float32), self.sample_rate, rate,
                                                        n_out, mix, self._mix_scale, pair["k"], layout="rows", want_stem=want_y)
                if pair["normalise"]:
                    c = eng.normalize(c, thr, amp)
            for source in (pair["model"], pair["complement"]):
                self._dev_stems.pop(id(source), None)
            kept, waiting = (c, y) if role == "complement" else (y, c)
            pair["converted"] = (where, waiting)
            if not other_wanted:
                self._complement = None
        if where == "host":
            return kept.T
        out = np.broadcast_to(np.float32(0), (n_out, 2))          # stands for the shape only: the writers read the device tensor
        self._dev_stems[id(out)] = (out, kept, None, "planar")
        return out

    def _stereo_rows(self, stem_source):
        a = np.asarray(stem_source)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"write_audio expects a [N, 2] stem, got {a.shape}")
        return a

    def _flac_on_device(self, stem_path: str) -> bool:
        """whether this stem is compressed by the engine's FLAC encoder: a ``.flac`` path, and pydub absent or ``asx_output_encoder`` = "device" """
        if stem_path.lower().split(".")[-1] != "flac":
            return False
        pydub = audio_io._optional("pydub")
        has_pydub = pydub is not None and hasattr(pydub, "AudioSegment") and hasattr(pydub.AudioSegment, "export")
        return not has_pydub or getattr(self, "asx_output_encoder", "host") == "device"

    def _write_flac_device(self, stem_path: str, pcm_dev, pcm_host, n: int, depth):
        """One ``.flac`` stem through asx_flac_encode_dev: ``pcm_dev`` (a device int16 tensor [n, 2]; the samples stay in HBM, only the
        compressed frames and their size table come back) or ``pcm_host`` (int16 [n, 2], uploaded by the engine).  An input of 24 or 32
        bits gives a 24-bit stream of v << 8 (ffmpeg's -sample_fmt s32 for the reference), anything else a 16-bit one.  The container
        is written on the WAV writer's worker threads; the MD5 of STREAMINFO is taken there when the samples are on the host, and left
        unset (zero, "not computed") for samples that never left the device."""
        eng = self.engine
        bits = 24 if depth in (24, 32) else 16
        block = getattr(eng, "FLAC_BLOCK_SIZE", 4096)
        t0 = self._now()
        if pcm_dev is not None:
            import torch
            plan = eng.flac_plan(n, 2, bits, block)
            out = torch.empty(plan["max_bytes"], dtype=torch.uint8, device=pcm_dev.device)
            sizes = torch.empty(plan["n_blocks"], dtype=torch.int32, device=pcm_dev.device)
            total = eng.flac_encode_dev(pcm_dev.data_ptr(), n, self._container_rate(), bits, block, out.data_ptr(), plan["max_bytes"], sizes.data_ptr(),
                                        stream=self._stream())
            frames_host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            sizes_host = torch.empty(plan["n_blocks"], dtype=torch.int32, pin_memory=True)
            frames_host.copy_(out[:total], non_blocking=True)
            sizes_host.copy_(sizes, non_blocking=True)
            self._sync()
            frames, frame_sizes = frames_host.numpy(), sizes_host.numpy()
            self.last_write_path = "flac_device_resident"
        else:
            frames, frame_sizes = eng.flac_encode(pcm_host, self._container_rate(), bits, block)
            self.last_write_path = "flac_device_upload"
        self.file_timings["flac_encode"] = self.file_timings.get("flac_encode", 0.0) + (self._now() - t0)
        rate = self._container_rate()

        def write():
            md5 = None
            if pcm_host is not None:
                import hashlib
                raw = pcm_host if bits == 16 else (pcm_host.astype(np.int32) << 8)
                body = np.ascontiguousarray(raw.astype("<i2" if bits == 16 else "<i4", copy=False))
                if bits == 24:
                    body = np.ascontiguousarray(body.view(np.uint8).reshape(-1, 4)[:, :3])
                md5 = hashlib.md5(memoryview(body).cast("B")).digest()
            audio_io.write_flac(stem_path, frames, frame_sizes, rate, bits, n, md5, block_size=block)
        self._write_async(write)

    def write_audio_pydub(self, stem_path: str, stem_source):
        """common_separator.py:305-397.  normalize -> silence check -> (x * 32767).astype(int16) -> interleave is one
        device pass (asx_pcm16, bit-exact); the container is written by pydub when it is installed, else by the
        built-in WAV writer (int16 widened exactly like ffmpeg's s16 -> s32 / pcm_s24le conversion) or, for a ``.flac``
        path, by the engine's FLAC encoder and audio_io.write_flac (also with pydub when ``asx_output_encoder`` is "device")."""
        eng = self._require_engine()
        a = self._stereo_rows(stem_source)
        t0 = self._now()
        flac_dev = self._flac_on_device(stem_path)
        pcm_dev = None
        entry = self._device_stem_entry(stem_source)
        dev_stem = entry[1] if entry is not None else None
        if dev_stem is not None:
            # the stem is still in HBM (same array object separate() produced): normalise + quantise there, bring back int16 only
            import torch
            planar = entry[3] == "planar"                     # [2, N] (Demucs / MDXC stems) or [N, 2] (asx_separate_dev)
            n = dev_stem.shape[1] if planar else dev_stem.shape[0]
            pcm_dev = torch.empty((n, 2), dtype=torch.int16, device=dev_stem.device)
            quantise = eng.pcm16_planar_dev if planar else eng.pcm16_rows_dev
            peak = quantise(dev_stem.data_ptr(), n, self.normalization_threshold, self.amplification_threshold,
                            pcm_dev.data_ptr(), stream=self._stream())
            self._tap_stem(dev_stem, entry[3], n, pcm_dev, "PCM_16", peak)
            pcm = None
            if not flac_dev:                                  # (the FLAC encoder reads the int16 where it is)
                pcm_host = torch.empty((n, 2), dtype=torch.int16, pin_memory=True)
                pcm_host.copy_(pcm_dev, non_blocking=True)
                self._sync()
                pcm = pcm_host.numpy()
                pcm_dev = None
            # written: the device stem and its pinned mirror are released with this entry (planar stems share one mirror, which
            # lives until the last of them is written)
            self._dev_stems.pop(id(stem_source), None)
        elif a.dtype == np.int16:
            pcm, peak = np.ascontiguousarray(a), float(np.abs(a).max()) if a.size else 0.0
        else:
            if a.shape[0] == 0:
                self.logger.warning(f"{stem_path}: nothing to write (the stem is empty or silent)")
                return
            pcm, peak = eng.pcm16(a, self.normalization_threshold, self.amplification_threshold)
        t0 = self._tick("pcm16_d2h", t0)
        if peak < 1e-6:
            self.logger.warning(f"{stem_path}: nothing to write (the stem is empty or silent)")
            return
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            stem_path = os.path.join(self.output_dir, stem_path)
        depth = self.input_bit_depth if self.input_bit_depth is not None else 16
        self.logger.info(f"{stem_path}: {depth}-bit output (the input's bit depth)")
        file_format = stem_path.lower().split(".")[-1]
        if flac_dev:
            self._write_flac_device(stem_path, pcm_dev, pcm, a.shape[0], depth)
            self._tick("container_write", t0)
            return
        pydub = audio_io._optional("pydub")
        if pydub is not None and hasattr(pydub, "AudioSegment") and hasattr(pydub.AudioSegment, "export"):
            seg = pydub.AudioSegment(pcm.reshape(-1).tobytes(), frame_rate=self._container_rate(), sample_width=2, channels=2)
            fmt = {"m4a": "mp4", "mka": "matroska"}.get(file_format, file_format)
            params = {"format": fmt}
            bitrate = "320k" if fmt == "mp3" and self.output_bitrate is None else self.output_bitrate
            if bitrate:
                params["bitrate"] = bitrate
            if fmt in ("wav", "flac"):
                if depth == 16:
                    params["parameters"] = ["-sample_fmt", "s16"]
                else:
                    params["parameters"] = ["-sample_fmt", "s32"]
                    if fmt == "wav":
                        params["codec"] = "pcm_s24le" if depth == 24 else "pcm_s32le"
            try:
                seg.export(stem_path, **params)
            except (IOError, ValueError) as e:
                self.logger.error(f"{stem_path}: the container write failed: {e}")
            return
        if file_format != "wav":
            raise audio_io.AudioIOError(f"writing .{file_format} needs pydub + ffmpeg (not installed); WAV and FLAC are built in")
        self._write_wav_async(stem_path, pcm, {16: "PCM_16", 24: "PCM_24", 32: "PCM_32"}.get(depth, "PCM_16"))
        self._tick("container_write", t0)

    def _output_subtype(self) -> str:
        """the sample format write_audio_soundfile keeps: the input's (common_separator.py:425-437)"""
        if self.input_subtype:
            return self.input_subtype
        if self.input_bit_depth:
            return {16: "PCM_16", 24: "PCM_24", 32: "PCM_32"}.get(self.input_bit_depth, "PCM_16")
        return "PCM_16"

    _DEVICE_WAV_SUBTYPES = {"PCM_16": 4, "PCM_24": 6, "PCM_32": 8, "FLOAT": 8}     # bytes per stereo frame
    _DEVICE_FLAC_SUBTYPES = {"PCM_16": (16, "S16_IN_32"), "PCM_24": (24, "S24_IN_32")}

    def _write_soundfile_device(self, stem_path: str, stem_source, entry) -> bool:
        """write_audio_soundfile for a stem that is still in HBM (``entry`` of ``_dev_stems``): normalise and convert to the file's own
        sample format there (asx_pcm_encode_dev), bring back the file's bytes -- or, for a ``.flac`` name, its compressed frames
        (asx_flac_encode_pcm_dev: a PCM_24 input keeps 24 real bits) -- and write the container on the writer threads.  False: not a case
        of this path (another container, a subtype without a device encoder, soundfile installed and not overruled); the caller goes on."""
        if not self._soundfile_on_device(stem_path):
            return False
        eng = self.engine
        file_format = stem_path.lower().split(".")[-1]
        subtype = self._output_subtype()
        if file_format == "flac" and subtype not in self._DEVICE_FLAC_SUBTYPES:
            # what sf.write does under the reference: libsndfile's FLAC takes neither 32-bit nor float samples
            self.logger.error(f"{stem_path}: the container write failed: FLAC holds no {subtype} samples")
            self._dev_stems.pop(id(stem_source), None)
            return True
        import torch
        dev_stem = entry[1]
        layout = "planar" if entry[3] == "planar" else "rows"
        n = dev_stem.shape[1] if layout == "planar" else dev_stem.shape[0]
        t0 = self._now()
        if file_format == "wav":
            fmt, dev_body = subtype, torch.empty(n * self._DEVICE_WAV_SUBTYPES[subtype], dtype=torch.uint8, device=dev_stem.device)
        else:
            bits, fmt = self._DEVICE_FLAC_SUBTYPES[subtype]
            dev_body = torch.empty((n, 2), dtype=torch.int32, device=dev_stem.device)
        peak = eng.pcm_encode_dev(dev_stem.data_ptr(), n, layout, self.normalization_threshold, self.amplification_threshold, fmt,
                                  dev_body.data_ptr(), stream=self._stream())
        self._tap_stem(dev_stem, layout, n, dev_body if file_format == "wav" else None, subtype, peak)
        # written (or silent): the device stem and its pinned mirror are released with this entry, as in write_audio_pydub
        self._dev_stems.pop(id(stem_source), None)
        if peak < 1e-6:
            self.logger.warning(f"{stem_path}: nothing to write (the stem is empty or silent)")
            return True
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            stem_path = os.path.join(self.output_dir, stem_path)
        rate = self._container_rate()
        if file_format == "wav":
            body = torch.empty(dev_body.shape, dtype=torch.uint8, pin_memory=True)
            body.copy_(dev_body, non_blocking=True)
            self._sync()
            self.file_timings["pcm_encode_d2h"] = self.file_timings.get("pcm_encode_d2h", 0.0) + (self._now() - t0)
            self.last_write_path = "wav_device_resident"
            self._write_async(lambda: audio_io.write_wav_body(stem_path, body.numpy(), rate, subtype, n))
            return True
        self.file_timings["pcm_encode_d2h"] = self.file_timings.get("pcm_encode_d2h", 0.0) + (self._now() - t0)
        t0 = self._now()
        block = getattr(eng, "FLAC_BLOCK_SIZE", 4096)
        plan = eng.flac_plan_pcm(n, 2, bits, block)
        out = torch.empty(plan["max_bytes"], dtype=torch.uint8, device=dev_stem.device)
        sizes = torch.empty(plan["n_blocks"], dtype=torch.int32, device=dev_stem.device)
        total = eng.flac_encode_pcm_dev(dev_body.data_ptr(), n, rate, bits, block, out.data_ptr(), plan["max_bytes"], sizes.data_ptr(),
                                        stream=self._stream())
        frames = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        frame_sizes = torch.empty(plan["n_blocks"], dtype=torch.int32, pin_memory=True)
        frames.copy_(out[:total], non_blocking=True)
        frame_sizes.copy_(sizes, non_blocking=True)
        self._sync()
        self.file_timings["flac_encode"] = self.file_timings.get("flac_encode", 0.0) + (self._now() - t0)
        self.last_write_path = "flac_device_resident"
        # the MD5 of STREAMINFO stays unset ("not computed"): the samples never reached the host
        self._write_async(lambda: audio_io.write_flac(stem_path, frames.numpy(), frame_sizes.numpy(), rate, bits, n, None, block_size=block))
        return True

    def write_audio_soundfile(self, stem_path: str, stem_source):
        """common_separator.py:399-461: normalise (device), keep the input's subtype, hand floats to the container.  A stem that is still
        in HBM is converted to the file's format there (``_write_soundfile_device``)."""
        eng = self._require_engine()
        a = self._stereo_rows(stem_source)
        if a.shape[0] == 0:
            self.logger.warning(f"{stem_path}: nothing to write (the stem is empty or silent)")
            return
        entry = self._device_stem_entry(stem_source)
        if entry is not None and self._write_soundfile_device(stem_path, stem_source, entry):
            return
        buf = eng.normalize(np.ascontiguousarray(a, np.float32), self.normalization_threshold, self.amplification_threshold)
        if np.max(np.abs(buf)) < 1e-6:
            self.logger.warning(f"{stem_path}: nothing to write (the stem is empty or silent)")
            return
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            stem_path = os.path.join(self.output_dir, stem_path)
        if self.input_subtype:
            subtype = self.input_subtype
        elif self.input_bit_depth:
            subtype = {16: "PCM_16", 24: "PCM_24", 32: "PCM_32"}.get(self.input_bit_depth, "PCM_16")
        else:
            subtype = "PCM_16"
        sf = audio_io._optional("soundfile")
        try:
            if sf is not None and hasattr(sf, "write"):
                sf.write(stem_path, buf, self._container_rate(), subtype=subtype)
            else:
                audio_io.write_wav(stem_path, buf, self._container_rate(), subtype)
        except Exception as e:
            self.logger.error(f"{stem_path}: the container write failed: {e}")

    # ---- per-file state ------------------------------------------------------
    def clear_gpu_cache(self):
        """common_separator.py:463-474.  The engine's workspaces are sized once and reused across files (they are the
        point of keeping 288 GB resident); only Python garbage and torch's caching allocator are trimmed."""
        self._dev_stems = {}
        self._out_rate_group = None
        self._file_mix, self._complement = None, None
        gc.collect()
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.empty_cache()
        except Exception:
            pass

    def clear_file_specific_paths(self):
        """common_separator.py:476-489."""
        self.logger.info("per-file state reset (paths, sources, stems)")
        self._reset_file_state()

    # ---- file naming -------------------------------------------------------
    def sanitize_filename(self, filename):
        """common_separator.py:491-498."""
        s = re.sub(r'[<>:"/\\|?*]', "_", filename)
        s = re.sub(r"_+", "_", s)
        return s.strip("_. ")

    def get_stem_output_path(self, stem_name, custom_output_names):
        """common_separator.py:500-519: names are relative to ``output_dir``."""
        ext = self.output_format.lower()
        if custom_output_names:
            lowered = {k.lower(): v for k, v in custom_output_names.items()}
            if stem_name.lower() in lowered:
                return os.path.join(f"{self.sanitize_filename(lowered[stem_name.lower()])}.{ext}")
        return os.path.join(f"{self.sanitize_filename(self.audio_file_base)}_({self.sanitize_filename(stem_name)})_"
                            f"{self.sanitize_filename(self.model_name)}.{ext}")

    # ---- Roformer hooks the orchestrator probes (separator.py:926-929) -------
    def _detect_roformer_model(self):
        """common_separator.py:521-543."""
        if not self.model_data:
            return False
        if self.model_data.get("is_roformer", False):
            return True
        for text in (self.model_path, self.model_name):
            if text and "roformer" in text.lower():
                return True
        return False

    def _initialize_roformer_loader(self):
        from .roformer_config import RoformerLoader
        self.roformer_loader = RoformerLoader()

    def get_roformer_loading_stats(self):
        return self.roformer_loader.get_loading_stats() if self.roformer_loader else {}

    def validate_roformer_config(self, config, model_type):
        return self.roformer_loader.validate_configuration(config, model_type) if self.roformer_loader else True


# Derived stem tables (class scope cannot see the table from inside a comprehension, hence here).  STEM_PAIR_MAPPER: the pairs
# that name each other's complement -- any other stem X is complemented by "No X" (CommonSeparator.secondary_stem);
# NON_ACCOM_STEMS: stems that are not an accompaniment mix (common_separator.py:49-53).
_L = CommonSeparator._STEM_LABELS
CommonSeparator.STEM_PAIR_MAPPER = {_L[a]: _L[b] for a, b in (("VOCAL_STEM", "INST_STEM"), ("LEAD_VOCAL_STEM", "BV_VOCAL_STEM"),
                                                              ("PRIMARY_STEM", "SECONDARY_STEM"))}
CommonSeparator.STEM_PAIR_MAPPER.update({v: k for k, v in list(CommonSeparator.STEM_PAIR_MAPPER.items()) if v != _L["SECONDARY_STEM"]})
CommonSeparator.NON_ACCOM_STEMS = tuple(_L[k] for k in ("VOCAL_STEM", "OTHER_STEM", "BASS_STEM", "DRUM_STEM", "GUITAR_STEM", "PIANO_STEM",
                                                         "SYNTH_STEM", "STRINGS_STEM", "WOODWINDS_STEM", "BRASS_STEM", "WIND_INST_STEM"))
del _L
