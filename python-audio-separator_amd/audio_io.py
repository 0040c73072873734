"""File edges of the plugin surface: decode and encode stay on the host ("boundary, stays host").

The reference decodes with ``librosa.load`` and encodes with pydub (ffmpeg) or soundfile
(common_separator.py:217-282, 284-461).  When those packages are installed they are used here too, unchanged.
When they are not (this image ships none of them), RIFF/WAVE files -- integer PCM 8/16/24/32 and IEEE float
32/64, plain or WAVE_FORMAT_EXTENSIBLE -- are read and written by the small codec below so that
``separate(path) -> [file names]`` works end to end; every other container then raises with the name of the
missing package.  Nothing here touches the GPU: the sample arithmetic of the writer (normalise, * 32767,
int16 cast, interleave) is ``asx_pcm16`` (include/asx.h), called by CommonSeparator.  FLAC output needs no package either:
the audio frames come from the device encoder (``asx_flac_encode_dev``) and ``write_flac`` puts the container around them.
"""
from __future__ import annotations

import os
import struct

import numpy as np

_FMT_PCM, _FMT_FLOAT, _FMT_EXT = 1, 3, 0xFFFE


class AudioIOError(RuntimeError):
    pass


def _optional(name):
    try:
        return __import__(name)
    except Exception:
        return None


def _riff_chunks(f):
    head = f.read(12)
    if len(head) < 12 or head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
        raise AudioIOError("not a RIFF/WAVE file")
    while True:
        h = f.read(8)
        if len(h) < 8:
            return
        cid, size = h[:4], struct.unpack("<I", h[4:])[0]
        pos = f.tell()
        yield cid, size, pos
        f.seek(pos + size + (size & 1))


def wav_info(path: str) -> dict:
    """{samplerate, channels, frames, subtype} with soundfile's subtype names (PCM_16, PCM_24, PCM_32, PCM_U8, FLOAT, DOUBLE)."""
    with open(path, "rb") as f:
        fmt = None
        for cid, size, pos in _riff_chunks(f):
            if cid == b"fmt ":
                raw = f.read(min(size, 40))
                tag, ch, sr, _, align, bits = struct.unpack("<HHIIHH", raw[:16])
                if tag == _FMT_EXT and len(raw) >= 26:
                    tag = struct.unpack("<H", raw[24:26])[0]
                fmt = (tag, ch, sr, align, bits)
            elif cid == b"data":
                if fmt is None:
                    raise AudioIOError("data chunk before fmt chunk")
                tag, ch, sr, align, bits = fmt
                size = min(size, os.path.getsize(path) - pos)
                if tag == _FMT_PCM and bits in (8, 16, 24, 32):
                    subtype = {8: "PCM_U8", 16: "PCM_16", 24: "PCM_24", 32: "PCM_32"}[bits]
                elif tag == _FMT_FLOAT and bits in (32, 64):
                    subtype = "FLOAT" if bits == 32 else "DOUBLE"
                else:
                    raise AudioIOError(f"unsupported WAVE encoding (format tag {tag}, {bits} bits)")
                return {"samplerate": sr, "channels": ch, "frames": size // max(align, 1), "subtype": subtype,
                        "data_offset": pos, "data_bytes": size, "bits": bits}
    raise AudioIOError("no data chunk")


def read_wav(path: str):
    """(float32 [channels, frames], samplerate); integer PCM is scaled by 2^-(bits-1) like libsndfile / audioread."""
    info = wav_info(path)
    ch, bits = info["channels"], info["bits"]
    with open(path, "rb") as f:
        f.seek(info["data_offset"])
        raw = f.read(info["frames"] * ch * bits // 8)
    st = info["subtype"]
    if st == "PCM_16":
        x = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    elif st == "PCM_24":
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16))
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = (v.astype(np.float64) / 8388608.0).astype(np.float32)
    elif st == "PCM_32":
        x = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif st == "PCM_U8":
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
    elif st == "FLOAT":
        x = np.frombuffer(raw, "<f4").astype(np.float32)
    else:
        x = np.frombuffer(raw, "<f8").astype(np.float32)
    return np.ascontiguousarray(x.reshape(-1, ch).T), info["samplerate"]


def write_wav(path: str, data: np.ndarray, samplerate: int, subtype: str = "PCM_16"):
    """data: [frames, channels] (or [frames]); int16 input is widened bit-exactly (what ffmpeg's s16 -> s32 / pcm_s24le
    conversion does, common_separator.py:375-391), float input is rounded to the target width with clipping."""
    a = np.asarray(data)
    if a.ndim == 1:
        a = a[:, None]
    frames, ch = a.shape
    if subtype in ("FLOAT", "DOUBLE"):
        body = a.astype("<f4" if subtype == "FLOAT" else "<f8").tobytes()
        tag, bits = _FMT_FLOAT, 32 if subtype == "FLOAT" else 64
    else:
        bits = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32}.get(subtype)
        if bits is None:
            raise AudioIOError(f"unsupported WAV subtype {subtype}")
        if a.dtype == np.int16 and bits == 16:
            v = None                                   # already the file's sample format: no widening pass
        elif a.dtype == np.int16:
            v = a.astype(np.int32) << (bits - 16)
        else:
            full = float(2 ** (bits - 1) - 1)
            v = np.clip(np.rint(a.astype(np.float64) * full), -full - 1, full).astype(np.int64)
        if v is None:
            body = memoryview(np.ascontiguousarray(a.astype("<i2", copy=False))).cast("B")
        elif bits == 16:
            body = v.astype("<i2").tobytes()
        elif bits == 32:
            body = v.astype("<i4").tobytes()
        else:
            u = (v & 0xFFFFFF).astype(np.uint32).reshape(-1)
            body = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
        tag = _FMT_PCM
    _write_riff(path, tag, ch, samplerate, bits, body)


def _write_riff(path, tag, ch, samplerate, bits, body):
    align = ch * bits // 8
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, tag, ch, samplerate, samplerate * align, align, bits))
        f.write(b"data" + struct.pack("<I", len(body)))
        f.write(body)


_WAV_BODY_FORMATS = {"PCM_16": (_FMT_PCM, 16), "PCM_24": (_FMT_PCM, 24), "PCM_32": (_FMT_PCM, 32), "FLOAT": (_FMT_FLOAT, 32)}


def write_wav_body(path: str, body, samplerate: int, subtype: str, frames: int, channels: int = 2):
    """The file ``write_wav`` writes, around samples that are already in the file's format (Engine.pcm_encode*): ``body`` (bytes-like) is
    the data chunk of ``frames`` interleaved frames, little-endian, at ``subtype`` PCM_16 / PCM_24 (3-byte packed) / PCM_32 / FLOAT."""
    if subtype not in _WAV_BODY_FORMATS:
        raise AudioIOError(f"unsupported WAV subtype {subtype}")
    tag, bits = _WAV_BODY_FORMATS[subtype]
    body = body if isinstance(body, (bytes, bytearray)) else memoryview(body).cast("B")
    align = channels * bits // 8
    if len(body) != frames * align:
        raise AudioIOError(f"write_wav_body: {frames} frames of {align} bytes are {frames * align} bytes, the body holds {len(body)}")
    if 36 + len(body) >= 1 << 32:
        raise AudioIOError("write_wav_body: the body does not fit a RIFF file's 32-bit sizes")
    _write_riff(path, tag, channels, samplerate, bits, body)


def write_flac(path: str, frames, frame_sizes, samplerate: int, bits_per_sample: int, total_samples: int, md5=None,
               block_size: int = 4096, channels: int = 2):
    """A .flac file around audio frames that are already coded (Engine.flac_encode*): the marker, one STREAMINFO block (the last
    metadata block) and ``frames`` (bytes-like, the frames back to back).  STREAMINFO: minimum = maximum block size ``block_size``
    (a fixed-blocksize stream; only the last frame may be shorter), the smallest and largest entry of ``frame_sizes``, sample rate,
    channels, bits per sample, ``total_samples`` inter-channel samples, and ``md5``: the 16-byte digest of the little-endian
    interleaved PCM at the stream's sample width, or None = not computed (sixteen zero bytes, as the format provides)."""
    sizes = np.asarray(frame_sizes, np.int64).reshape(-1)
    if sizes.size == 0 or total_samples < 1:
        raise AudioIOError("write_flac: no frames")
    if not (1 <= samplerate < 1 << 20 and 1 <= channels <= 8 and 4 <= bits_per_sample <= 32 and total_samples < 1 << 36):
        raise AudioIOError("write_flac: stream parameters outside what STREAMINFO holds")
    body = memoryview(frames).cast("B") if not isinstance(frames, (bytes, bytearray)) else frames
    if int(sizes.sum()) != len(body):
        raise AudioIOError(f"write_flac: the size table sums to {int(sizes.sum())} bytes, the frames are {len(body)}")
    digest = bytes(16) if md5 is None else bytes(md5)
    if len(digest) != 16:
        raise AudioIOError("write_flac: md5 must be 16 bytes")
    packed = (samplerate << 44) | ((channels - 1) << 41) | ((bits_per_sample - 1) << 36) | int(total_samples)
    info = struct.pack(">HH", block_size, block_size) + min(int(sizes.min()), 0xFFFFFF).to_bytes(3, "big") + \
        min(int(sizes.max()), 0xFFFFFF).to_bytes(3, "big") + packed.to_bytes(8, "big") + digest
    with open(path, "wb") as f:
        f.write(b"fLaC" + bytes([0x80]) + len(info).to_bytes(3, "big") + info)
        f.write(body)


def flac_info(path: str) -> dict:
    """{samplerate, channels, frames, subtype} from the STREAMINFO block of a .flac file"""
    with open(path, "rb") as f:
        head = f.read(8 + 34)
    if len(head) < 42 or head[:4] != b"fLaC" or head[4] & 127 != 0:
        raise AudioIOError("not a FLAC file (no marker, or STREAMINFO is not its first block)")
    v = int.from_bytes(head[18:26], "big")
    bits = ((v >> 36) & 31) + 1
    return {"samplerate": v >> 44, "channels": ((v >> 41) & 7) + 1, "frames": v & ((1 << 36) - 1),
            "subtype": {8: "PCM_S8", 16: "PCM_16", 24: "PCM_24"}.get(bits, f"PCM_{bits}"), "bits": bits}


def _id3v2_size(head: bytes) -> int:
    """bytes of an ID3v2 tag at the start of ``head`` (10 bytes of header with a sync-safe size, plus a footer when flagged), or 0"""
    if len(head) < 10 or head[:3] != b"ID3" or any(b & 0x80 for b in head[6:10]):
        return 0
    size = (head[6] << 21) | (head[7] << 14) | (head[8] << 7) | head[9]
    return 10 + size + (10 if head[5] & 0x10 else 0)


def is_flac(path: str) -> bool:
    """True when the file carries the fLaC marker, at its start or behind an ID3v2 tag (the extension is not looked at)"""
    try:
        with open(path, "rb") as f:
            head = f.read(10)
            if head[:4] == b"fLaC":
                return True
            skip = _id3v2_size(head)
            if not skip:
                return False
            f.seek(skip)
            return f.read(4) == b"fLaC"
    except OSError:
        return False


def flac_stream(path: str) -> dict:
    """A native FLAC file as the device decoder needs it: STREAMINFO's fields {min_blocksize, max_blocksize, min_framesize, max_framesize,
    samplerate, channels, bits_per_sample, total_samples (a hint: 0 = unknown), md5} plus audio_offset and audio_bytes -- the audio
    frames are everything behind the last metadata block, to the end of the file.  An ID3v2 tag in front of the marker is skipped; any
    number and kind of metadata blocks may follow STREAMINFO."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pos = _id3v2_size(f.read(10))
        f.seek(pos)
        if f.read(4) != b"fLaC":
            raise AudioIOError("not a FLAC file (no fLaC marker)")
        pos += 4
        fields, first = None, True
        while True:
            head = f.read(4)
            if len(head) < 4:
                raise AudioIOError("FLAC metadata runs past the end of the file")
            kind, length = head[0] & 127, int.from_bytes(head[1:4], "big")
            if first:
                body = f.read(34)
                if kind != 0 or length != 34 or len(body) != 34:
                    raise AudioIOError("not a FLAC file (STREAMINFO is not its first block)")
                v = int.from_bytes(body[10:18], "big")
                fields = {"min_blocksize": int.from_bytes(body[0:2], "big"), "max_blocksize": int.from_bytes(body[2:4], "big"),
                          "min_framesize": int.from_bytes(body[4:7], "big"), "max_framesize": int.from_bytes(body[7:10], "big"),
                          "samplerate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits_per_sample": ((v >> 36) & 31) + 1,
                          "total_samples": v & ((1 << 36) - 1), "md5": bytes(body[18:34])}
                first = False
            pos += 4 + length
            if pos > size:
                raise AudioIOError("FLAC metadata runs past the end of the file")
            f.seek(pos)
            if head[0] & 0x80:
                break
    fields.update(audio_offset=pos, audio_bytes=size - pos)
    return fields


def info(path: str) -> dict:
    """soundfile.info's fields the plugin reads (subtype; common_separator.py:233-250, vr_separator.py:137-156)."""
    sf = _optional("soundfile")
    if sf is not None:
        i = sf.info(path)
        return {"samplerate": i.samplerate, "channels": i.channels, "frames": i.frames, "subtype": i.subtype}
    if isinstance(path, str) and path.lower().endswith(".flac"):
        return flac_info(path)
    return wav_info(path)


def duration(path: str) -> float:
    try:
        i = info(path)
        return i["frames"] / float(i["samplerate"])
    except Exception:
        return 0.0


def load(path: str, sr: int | None = 44100, mono: bool = False, res_type: str | None = None):
    """librosa.load(path, sr=sr, mono=mono) (common_separator.py:252): float32 [channels, n] (or [n] for a mono file)."""
    librosa = _optional("librosa")
    if librosa is not None and hasattr(librosa, "load"):
        kw = {"res_type": res_type} if res_type else {}
        return librosa.load(path, mono=mono, sr=sr, **kw)
    try:
        x, file_sr = read_wav(path)
    except AudioIOError as e:
        if isinstance(path, str) and is_flac(path):
            try:
                file_sr = flac_stream(path)["samplerate"]
            except AudioIOError:
                file_sr = None
            if sr is not None and file_sr is not None and file_sr != sr:
                raise AudioIOError(f"{path} is sampled at {file_sr} Hz and librosa (which resamples to {sr} Hz on load) is not installed") from e
            raise AudioIOError(f"{path}: FLAC is decoded on the device (the file fast path of the separators, 16- or 24-bit mono / stereo "
                               f"streams); this host loader reads RIFF/WAVE only -- install librosa (+ soundfile) for a host decode") from e
        raise AudioIOError(f"{path}: {e}; install librosa (+ soundfile / audioread) to decode other containers") from e
    if sr is not None and file_sr != sr:
        raise AudioIOError(f"{path} is sampled at {file_sr} Hz and librosa (which resamples to {sr} Hz on load) is not installed")
    if x.shape[0] == 1:
        x = x[0]
    elif mono:
        x = x.mean(0)
    return x, file_sr
