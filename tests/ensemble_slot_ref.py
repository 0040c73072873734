"""The member -> Ensembler edge in numpy: what a stem becomes on its way through its member's writer and audio_io.load, per slot
mode of ``Engine.SLOT_MODES`` -- the restatement the slot and pooled-ensemble tests compare the engine with.

* spec_utils.normalize in float32, one rounding per operation (the scale is a float32 quotient, applied only outside the thresholds);
* "pcm16": pydub's writer, ``(x * 32767).astype(int16)`` in float32 (truncation), read back as ``int16 / 32768``;
* "PCM_16" / "PCM_24" / "PCM_32": the soundfile writer's file, ``clip(rint(float64(x) * (2^(b-1) - 1)))`` (ties to even), read back as
  ``int / 2^(b-1)`` (through float64, which only matters at 32 bits);
* "FLOAT": the normalised float itself; "float32": the stem as it is, no normalisation."""
import numpy as np

FILE_BITS = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32}
FILE_MODES = ("PCM_16", "PCM_24", "PCM_32", "FLOAT")


def normalize(x, max_peak, min_peak):
    """(normalised float32 copy of ``x``, peak after normalisation as float32); ``min_peak`` None: no amplification."""
    x = np.asarray(x, np.float32)
    maxv = np.float32(np.abs(x).max()) if x.size else np.float32(0.0)
    scale = None
    if maxv > np.float32(max_peak):
        scale = np.float32(max_peak) / maxv
    elif min_peak is not None and maxv < np.float32(min_peak):
        scale = np.float32(min_peak) / maxv
    if scale is None:
        return x.copy(), maxv
    scale = np.float32(scale)
    return (x * scale).astype(np.float32), np.float32(maxv * scale)


def file_integers(x, bits):
    """the integer samples of ``bits`` bits the soundfile writer stores for the normalised float32 ``x`` (int64 array)"""
    full = float((1 << (bits - 1)) - 1)
    return np.clip(np.rint(np.asarray(x, np.float32).astype(np.float64) * full), -full - 1.0, full).astype(np.int64)


def round_trip(x, mode, max_peak, min_peak):
    """(float32 array of ``x``'s shape as the Ensembler reads it back, peak_after)"""
    x = np.asarray(x, np.float32)
    if mode == "float32":
        return x.copy(), (np.float32(np.abs(x).max()) if x.size else np.float32(0.0))
    y, peak = normalize(x, max_peak, min_peak)
    if mode == "pcm16":
        q = (y * np.float32(32767.0)).astype(np.float32).astype(np.int16)
        return (q.astype(np.float32) / np.float32(32768.0)), peak
    if mode == "FLOAT":
        return y, peak
    bits = FILE_BITS[mode]
    return (file_integers(y, bits).astype(np.float64) / float(1 << (bits - 1))).astype(np.float32), peak


def slot_image(x, mode, max_peak, min_peak, n_max):
    """``x`` planar [2, n] -> (slot [2, n_max], zero from n on; peak_after)"""
    back, peak = round_trip(x, mode, max_peak, min_peak)
    slot = np.zeros((2, n_max), np.float32)
    slot[:, : back.shape[1]] = back
    return slot, peak
