"""A FLAC stream builder for the decoder's tests: a bit writer that makes frames from explicit descriptions (RFC 9639), so that every
subframe type, header code and residual coding the format allows can be put in front of a decoder, whether or not an encoder would choose
it.  The CRCs come from tests/flac_ref.py; tests/test_host_flac_synth.py pins every stream to flac_ref's decode.

A frame is a dict: blocksize, subframes (one per channel) and optionally bs_code (the header's block-size code; default: the table code
if there is one, else 6 / 7), variable, number (the coded frame or sample number; default: the running one), assignment, ss_code (the
sample-size code; default: from the width, 0 = "see STREAMINFO"), rate_code.  A subframe is a dict: type CONSTANT / VERBATIM / FIXED / LPC,
x (the subframe's channel: after the stereo decorrelation, before the wasted-bits shift is taken out), and for the predicted types order,
coefs, precision, shift, method, partition_order and params: per partition a Rice parameter, or ("esc", width).  wasted defaults to 0.
`stereo(l, r, assignment)` gives the two channels of an assignment."""
import struct

import numpy as np

from tests import flac_ref as F

FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BS_TABLE = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def u(self, value, width):
        value, width = int(value), int(width)
        if width:
            assert 0 <= value < (1 << width), (value, width)
            self.v = (self.v << width) | value
            self.n += width

    def s(self, value, width):
        value, width = int(value), int(width)
        if width:
            assert -(1 << (width - 1)) <= value < (1 << (width - 1)), (value, width)
            self.u(value & ((1 << width) - 1), width)

    def unary(self, zeros):
        zeros = int(zeros)
        self.v = (self.v << (zeros + 1)) | 1
        self.n += zeros + 1

    def align(self):
        pad = -self.n % 8
        self.v <<= pad
        self.n += pad

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def coded_number(n):
    if n < 0x80:
        return bytes([n])
    extra = next(e for e in range(1, 7) if n < 1 << (6 + 5 * e))
    out = [((0xFE << (6 - extra)) & 0xFF) | (n >> (6 * extra))]
    out += [0x80 | ((n >> (6 * i)) & 0x3F) for i in range(extra - 1, -1, -1)]
    return bytes(out)


def stereo(l, r, assignment):
    l, r = np.asarray(l, np.int64), np.asarray(r, np.int64)
    if assignment == 8:
        return [l, l - r]
    if assignment == 9:
        return [l - r, r]
    if assignment == 10:
        return [(l + r) >> 1, l - r]
    return [l, r]


def residual_of(x, coefs, shift):
    x = [int(v) for v in x]
    order = len(coefs)
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, len(x))]


def _subframe(w, sub, bs, bits):
    kind = sub["type"]
    order = sub.get("order", 0)
    wasted = sub.get("wasted", 0)
    x = [int(v) for v in sub["x"]]
    assert len(x) == bs and all(v % (1 << wasted) == 0 for v in x)
    x = [v >> wasted for v in x]
    bits -= wasted
    code = {"CONSTANT": 0, "VERBATIM": 1}.get(kind, (8 + order) if kind == "FIXED" else (31 + order))
    w.u(0, 1)
    w.u(code, 6)
    w.u(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    if kind == "CONSTANT":
        assert len(set(x)) == 1
        w.s(x[0], bits)
        return
    if kind == "VERBATIM":
        for v in x:
            w.s(v, bits)
        return
    for v in x[:order]:
        w.s(v, bits)
    if kind == "LPC":
        coefs, shift, precision = list(sub["coefs"]), sub["shift"], sub["precision"]
        assert len(coefs) == order
        w.u(precision - 1, 4)
        w.s(shift, 5)
        for c in coefs:
            w.s(c, precision)
    else:
        coefs, shift = FIXED[order], 0
    res = residual_of(x, coefs, shift)
    method, po = sub.get("method", 0), sub.get("partition_order", 0)
    params = sub.get("params", [0] * (1 << po))
    assert len(params) == 1 << po and bs % (1 << po) == 0 and (bs >> po) >= order
    w.u(method, 2)
    w.u(po, 4)
    pbits = 5 if method else 4
    at = 0
    for j, k in enumerate(params):
        n = (bs >> po) - (order if j == 0 else 0)
        part = res[at:at + n]
        at += n
        if isinstance(k, tuple):
            w.u((1 << pbits) - 1, pbits)
            w.u(k[1], 5)
            for v in part:
                if k[1]:
                    w.s(v, k[1])
                else:
                    assert v == 0
        else:
            assert k < (1 << pbits) - 1
            w.u(k, pbits)
            for v in part:
                u = (v << 1) ^ (v >> 63) if v >= 0 else ((-v) << 1) - 1
                assert u < 1 << 32
                w.unary(u >> k)
                w.u(u & ((1 << k) - 1), k)
    assert at == len(res)


def build_frame(fr, stream, number):
    bs, bps = fr["blocksize"], stream["bits_per_sample"]
    a = fr.get("assignment", len(fr["subframes"]) - 1)
    bs_code = fr.get("bs_code", BS_TABLE.get(bs) or (6 if bs <= 256 else 7))
    rate = stream["samplerate"]
    rate_code = fr.get("rate_code", stream.get("rate_code", RATE_CODES.get(rate, 0)))
    ss_code = fr.get("ss_code", stream.get("ss_code", SS_CODES.get(bps, 0)))
    head = bytes([0xFF, 0xF8 | (1 if fr.get("variable", stream.get("variable", False)) else 0), (bs_code << 4) | rate_code, (a << 4) | (ss_code << 1)])
    head += coded_number(fr.get("number", number))
    if bs_code == 6:
        head += bytes([bs - 1])
    elif bs_code == 7:
        head += struct.pack(">H", bs - 1)
    if rate_code == 12:
        head += bytes([rate // 1000])
    elif rate_code == 13:
        head += struct.pack(">H", rate)
    elif rate_code == 14:
        head += struct.pack(">H", rate // 10)
    head += bytes([F.crc8(head)])
    w = Bits()
    for c, sub in enumerate(fr["subframes"]):
        side = (a == 8 and c == 1) or (a == 9 and c == 0) or (a == 10 and c == 1)
        _subframe(w, sub, bs, bps + (1 if side else 0))
    w.align()
    body = head + w.bytes()
    return body + struct.pack(">H", F.crc16(body))


def pcm_of(fr):
    """the samples a frame description stands for: int64 [blocksize, channels]"""
    ch = [np.asarray([int(v) for v in s["x"]], np.int64) for s in fr["subframes"]]
    a = fr.get("assignment", len(ch) - 1)
    if a == 8:
        ch[1] = ch[0] - ch[1]
    elif a == 9:
        ch[0] = ch[0] + ch[1]
    elif a == 10:
        mid = (ch[0] << 1) | (ch[1] & 1)
        ch[0], ch[1] = (mid + ch[1]) >> 1, (mid - ch[1]) >> 1
    return np.stack(ch, 1)


def metadata_block(kind, body, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(body).to_bytes(3, "big") + body


def build_stream(frames, bits_per_sample=16, samplerate=44100, channels=2, prefix=b"", blocks=(), trailer=b"", total_samples=None,
                 max_framesize=None, **codes):
    """{file, audio_offset, audio_bytes, info, pcm [n, channels], n_frames, frame_offsets (in the audio part), bytes_consumed}.
    prefix: bytes in front of the marker (an ID3v2 tag); blocks: (type, body) metadata blocks after STREAMINFO; trailer: bytes after the
    last frame; codes: stream-wide rate_code, ss_code, variable."""
    stream = {"bits_per_sample": bits_per_sample, "samplerate": samplerate, **codes}
    coded, offsets, pcm, number, at = [], [], [], 0, 0
    for fr in frames:
        assert len(fr["subframes"]) == channels
        b = build_frame(fr, stream, number)
        offsets.append(at)
        at += len(b)
        coded.append(b)
        pcm.append(pcm_of(fr))
        number += fr["blocksize"] if fr.get("variable", stream.get("variable", False)) else 1
    sizes = [fr["blocksize"] for fr in frames]
    n = sum(sizes)
    lens = [len(b) for b in coded]
    packed = (samplerate << 44) | ((channels - 1) << 41) | ((bits_per_sample - 1) << 36) | (n if total_samples is None else total_samples)
    info = struct.pack(">HH", min(sizes[:-1] or sizes), max(sizes)) + min(lens).to_bytes(3, "big") + \
        (max(lens) if max_framesize is None else max_framesize).to_bytes(3, "big") + packed.to_bytes(8, "big") + bytes(16)
    meta = b"fLaC" + metadata_block(0, info, last=not blocks)
    for i, (kind, body) in enumerate(blocks):
        meta += metadata_block(kind, body, last=i == len(blocks) - 1)
    audio = b"".join(coded)
    return {"file": prefix + meta + audio + trailer, "audio_offset": len(prefix) + len(meta), "audio_bytes": len(audio) + len(trailer),
            "info": F.parse_streaminfo(info), "pcm": np.concatenate(pcm), "n_frames": len(frames), "frame_offsets": offsets,
            "bytes_consumed": len(audio), "marker_offset": len(prefix)}


def damaged(stream, j, how):
    """`stream` with frame j damaged -- "body": one bit flipped in the middle of the frame, "header": one bit of its fourth byte, "cut": the
    file ends in the middle of the frame.  What a decoder must return is frames 0 .. j - 1."""
    data = bytearray(stream["file"])
    first = stream["audio_offset"] + stream["frame_offsets"][j]
    ends = stream["frame_offsets"][1:] + [stream["bytes_consumed"]]
    size = ends[j] - stream["frame_offsets"][j]
    if how == "body":
        data[first + size // 2] ^= 0x10
    elif how == "header":
        data[first + 3] ^= 0x20
    else:
        del data[first + size // 2:]
    # the samples in front of frame j: block sizes are those of the undamaged stream
    out = dict(stream)
    n_before = stream["_blocks"][:j]
    out.update(file=bytes(data), audio_bytes=len(data) - stream["audio_offset"], pcm=stream["pcm"][:sum(n_before)], n_frames=j,
               bytes_consumed=stream["frame_offsets"][j])
    return out


# ---- the streams ----------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _noise(rng, n, bits):
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), n, dtype=np.int64)


def _smooth(rng, n, bits, step=40):
    x = np.cumsum(rng.integers(-step, step + 1, n, dtype=np.int64))
    return np.clip(x, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)


def _verb(x):
    return {"type": "VERBATIM", "x": x}


def _fixed(x, order, k=None, **kw):
    sub = {"type": "FIXED", "order": order, "x": x, **kw}
    if "params" not in sub:
        sub["params"] = [k if k is not None else 4] * (1 << sub.get("partition_order", 0))
    return sub


def _lpc(x, coefs, precision, shift, **kw):
    sub = {"type": "LPC", "order": len(coefs), "x": x, "coefs": list(coefs), "precision": precision, "shift": shift, **kw}
    if "params" not in sub:
        sub["params"] = [("esc", 31)] * (1 << sub.get("partition_order", 0))
    return sub


def _frames(subs_per_frame, **kw):
    return [{"blocksize": len(subs[0]["x"]), "subframes": subs, **kw} for subs in subs_per_frame]


def _make():
    S = {}
    r = _rng(1)

    def add(name, frames, **kw):
        s = build_stream(frames, **kw)
        s["_blocks"] = [fr["blocksize"] for fr in frames]
        S[name] = s

    # subframe types
    add("constant", _frames([[{"type": "CONSTANT", "x": [v] * 16} for v in (5, -7)], [{"type": "CONSTANT", "x": [v] * 16} for v in (-32768, 32767)]]))
    add("verbatim", _frames([[_verb(_noise(r, 192, 16)), _verb(_noise(r, 192, 16))] for _ in range(3)]))
    add("fixed_orders", _frames([[_fixed(_smooth(r, 256, 16), o, k=6), _fixed(_smooth(r, 256, 16), 4 - o, k=7)] for o in range(5)]))
    lpc = []
    for order, precision, shift in ((1, 1, 0), (1, 15, 15), (8, 15, 0), (8, 1, 15), (12, 15, 14), (12, 9, 3), (32, 15, 15), (32, 1, 0), (32, 15, 0)):
        subs = []
        for _ in range(2):
            coefs = r.integers(-(1 << (precision - 1)), 1 << (precision - 1), order)
            subs.append(_lpc(_smooth(r, 192, 16, 3) if shift == 0 and precision > 8 else _smooth(r, 192, 16), coefs, precision, shift, method=1))
        lpc.append(subs)
    add("lpc_orders", _frames(lpc))
    # 24-bit samples, order 32, 15-bit coefficients of one sign against samples of one sign: the sum passes 2^32 long before the shift
    big = [[_lpc(np.full(64, v, np.int64) - r.integers(0, 1000, 64), [c] * 32, 15, 15, method=1) for v, c in ((8388607, 16383), (-8388608 + 1000, -16384))]]
    assert max(abs(sum(16383 * int(v) for v in big[0][0]["x"][:32])), 1) > 1 << 32
    add("lpc_sum_over_32_bits", _frames(big), bits_per_sample=24)
    # residual coding
    add("rice0_k0_k14", _frames([[_fixed(r.integers(-3, 4, 64), 0, k=0), _fixed(_noise(r, 64, 16), 1, k=14)]]))
    wide = r.integers(-(1 << 30), 1 << 30, 32, dtype=np.int64)
    add("rice1_k30", _frames([[_fixed(wide >> 8, 0, k=30, method=1), _fixed(_smooth(r, 32, 16), 2, k=3, method=1)]]), bits_per_sample=24)
    esc = [_fixed(np.concatenate([np.zeros(16, np.int64), r.integers(-1, 1, 16), _noise(r, 16, 24), _smooth(r, 16, 16)]), 0, partition_order=2,
                  params=[("esc", 0), ("esc", 1), ("esc", 25), 5]),
           _fixed(np.concatenate([np.zeros(32, np.int64), r.integers(-1, 1, 32)]), 0, partition_order=1, method=1, params=[("esc", 0), ("esc", 1)])]
    add("escapes_0_1_25", _frames([esc]), bits_per_sample=24)
    add("partition_max", _frames([[_fixed(_smooth(r, 4096, 16), 0, partition_order=12, params=list(r.integers(3, 9, 4096))),
                                   _fixed(_smooth(r, 4096, 16), 2, partition_order=0, params=[6])]]))
    add("partition_first_empty", _frames([[_fixed(_smooth(r, 64, 16), 4, partition_order=4, params=list(r.integers(4, 9, 16))),
                                           _lpc(_smooth(r, 64, 16), [3, -1], 4, 1, partition_order=5, params=[("esc", 20)] + [9] * 31)]]))
    one = np.zeros(16, np.int64)
    one[7] = 2500                                     # zigzag 5000 at k = 0: a unary run of 5000 zeros
    add("long_unary_run", _frames([[_fixed(one, 0, k=0), _fixed(-one, 0, k=0)]]))
    # wasted bits
    add("wasted_bits", _frames([[_fixed(_smooth(r, 192, 15) << 1, 1, k=6, wasted=1), _verb(_noise(r, 192, 9) << 7) | {"wasted": 7}],
                                [{"type": "CONSTANT", "x": [256 * 3] * 192, "wasted": 8}, _fixed(_smooth(r, 192, 8) << 8, 2, k=4, wasted=8)]]))
    l = _smooth(r, 192, 15) << 1
    add("wasted_bits_side", [{"blocksize": 192, "assignment": 8, "subframes": [_fixed(l, 1, k=7), _fixed((l - (_smooth(r, 192, 14) << 1)), 0, k=8, wasted=1)]}])
    # channel assignments at the extremes
    for bits in (16, 24):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        L = np.array([lo, hi, lo, hi, 0, 1, -1, hi - 1] * 2, np.int64)
        R = np.array([hi, lo, lo, hi, 1, 0, 2, lo + 1] * 2, np.int64)
        frames = []
        for a in (1, 8, 9, 10):
            c = stereo(L, R, a)
            frames.append({"blocksize": 16, "assignment": a, "subframes": [_verb(c[0]), _verb(c[1])]})
        add(f"assignments_{bits}", frames, bits_per_sample=bits)
    add("mono", _frames([[_fixed(_smooth(r, 576, 16), 2, k=5)], [_verb(_noise(r, 576, 16))]]), channels=1)
    # sample widths through the header codes and through STREAMINFO
    for bits in (8, 12, 16, 20, 24):
        fr = _frames([[_fixed(_smooth(r, 192, bits, 3), 1, k=3), _verb(_noise(r, 192, bits))]])
        add(f"bits_{bits}", fr, bits_per_sample=bits)
        add(f"bits_{bits}_streaminfo", fr, bits_per_sample=bits, ss_code=0)
    # block sizes
    for bs in (16, 17, 255, 257, 4097, 192, 576, 4608, 256, 4096, 16384):
        fr = _frames([[_fixed(_smooth(r, bs, 16), 1, k=5), _fixed(_smooth(r, bs, 16), 0, k=9)]])
        add(f"block_{bs}", fr)
    add("block_256_as_extra", _frames([[_verb(_noise(r, 256, 16)), _verb(_noise(r, 256, 16))]], bs_code=6))
    var = []
    for bs, number in ((16, 0), (4096, 0x7F), (17, 0x80), (576, 0x7FF), (255, 0x800), (1152, 0xFFFF), (4097, 0x10000), (192, 0x1FFFFF), (2304, 0x200000),
                       (256, 0x3FFFFFF), (300, 0x4000000), (31, 0x7FFFFFFF), (1000, 0xFFFFFFFFF)):
        var.append({"blocksize": bs, "number": number, "subframes": [_fixed(_smooth(r, bs, 16), 1, k=5), _fixed(_smooth(r, bs, 16), 2, k=4)]})
    add("variable_blocks", var, variable=True)
    add("short_last_frame", _frames([[_fixed(_smooth(r, n, 16), 1, k=5), _fixed(_smooth(r, n, 16), 1, k=5)] for n in (1152, 1152, 1152, 301)]))
    for code, rate in ((12, 32000), (12, 255000), (13, 44101), (13, 1), (14, 655350), (14, 44100), (0, 12345)):
        add(f"rate_code_{code}_{rate}", _frames([[_verb(_noise(r, 64, 16)), _verb(_noise(r, 64, 16))]] * 2), samplerate=rate, rate_code=code)
    # a VERBATIM subframe whose samples spell a complete frame, byte aligned in the outer frame (header 6 bytes + 1 subframe header byte)
    inner = build_frame({"blocksize": 192, "subframes": [{"type": "CONSTANT", "x": [1] * 192}, {"type": "CONSTANT", "x": [2] * 192}]},
                        {"bits_per_sample": 16, "samplerate": 44100}, 3)
    assert len(inner) % 2 == 0
    words = np.frombuffer(inner, ">i2").astype(np.int64)
    x0 = np.concatenate([words, _noise(r, 192 - len(words), 16)])
    add("frame_inside_verbatim", _frames([[_verb(_noise(r, 192, 16)), _verb(_noise(r, 192, 16))], [_verb(x0), _verb(_noise(r, 192, 16))],
                                          [_verb(_noise(r, 192, 16)), _verb(_noise(r, 192, 16))]]))
    # containers
    plain = _frames([[_fixed(_smooth(r, 1152, 16), 2, k=5), _fixed(_smooth(r, 1152, 16), 1, k=6)] for _ in range(4)])
    tag = b"ID3\x04\x00\x00" + bytes([0, 0, 1, 44]) + bytes(range(172))      # syncsafe 172
    add("id3v2_prefix", plain, prefix=tag)
    add("metadata_blocks", plain, blocks=[(1, bytes(100)), (4, struct.pack("<I", 4) + b"test" + struct.pack("<I", 0)), (3, bytes(18 * 3))])
    add("total_samples_0", plain, total_samples=0)
    add("trailing_tag", plain, trailer=b"TAG" + bytes(125))
    add("max_framesize_0", plain, max_framesize=0)
    for how in ("body", "header", "cut"):
        for j in (0, 2, 3):
            S[f"damaged_{how}_{j}"] = damaged(S["max_framesize_0"] if how == "body" and j == 2 else S["metadata_blocks"], j, how)
    return S


_STREAMS = None


def streams():
    """name -> stream (built once; treat as read-only)"""
    global _STREAMS
    if _STREAMS is None:
        _STREAMS = _make()
    return _STREAMS


def audio(stream) -> bytes:
    return stream["file"][stream["audio_offset"]:]


def planar(stream):
    """the stream's samples as the decoder's mix holds them: int64 [2, n], a mono stream in both rows"""
    p = stream["pcm"]
    return np.ascontiguousarray((p if p.shape[1] == 2 else np.repeat(p, 2, 1)).T)
