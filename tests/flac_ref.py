"""An independent FLAC decoder in Python / numpy, written from the format description (RFC 9639), and an exact bit counter for a
fixed-predictors-only encoding.  It imports nothing from the package: it is the reference the device encoder's output is decoded with.

Covered: the metadata chain (STREAMINFO is parsed, other blocks are skipped), the frame header with its CRC-8, the frame's CRC-16,
CONSTANT / VERBATIM / FIXED / LPC subframes, wasted bits, Rice methods 0 and 1 with escape partitions, independent channels and the
three stereo decorrelations.

Speed: the entropy decode of a partition walks the unary terminators through a next-set-bit table (one list lookup per sample) and
gathers the low bits of all its samples with numpy; the predictors of all subframes of a stream are restored together, one numpy step
per sample index.
"""
import struct

import numpy as np


class FlacError(ValueError):
    pass


def _crc_table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    tab = []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data) -> int:
    c = 0
    for b in bytes(data):
        c = _T8[c ^ b]
    return c


def crc16(data) -> int:
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def parse_streaminfo(block: bytes) -> dict:
    if len(block) != 34:
        raise FlacError(f"STREAMINFO of {len(block)} bytes")
    min_bs, max_bs = struct.unpack(">HH", block[:4])
    min_fs, max_fs = int.from_bytes(block[4:7], "big"), int.from_bytes(block[7:10], "big")
    v = int.from_bytes(block[10:18], "big")
    return {"min_blocksize": min_bs, "max_blocksize": max_bs, "min_framesize": min_fs, "max_framesize": max_fs,
            "samplerate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits_per_sample": ((v >> 36) & 31) + 1,
            "total_samples": v & ((1 << 36) - 1), "md5": bytes(block[18:34])}


def parse_container(data: bytes):
    """(STREAMINFO dict, [(block type, offset of the block's body, length)], offset of the first audio frame)"""
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, info, blocks = 4, None, []
    while True:
        if pos + 4 > len(data):
            raise FlacError("metadata chain runs past the end")
        last, kind, size = data[pos] >> 7, data[pos] & 127, int.from_bytes(data[pos + 1:pos + 4], "big")
        blocks.append((kind, pos + 4, size))
        if kind == 0:
            info = parse_streaminfo(data[pos + 4:pos + 4 + size])
        pos += 4 + size
        if last:
            break
    if info is None or blocks[0][0] != 0:
        raise FlacError("STREAMINFO must be the first metadata block")
    return info, blocks, pos


class _Bits:
    """MSB-first reads from a bytes object at a bit position"""

    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos

    def u(self, n):
        if n == 0:
            return 0
        p = self.pos
        b0, b1 = p >> 3, (p + n + 7) >> 3
        if b1 > len(self.data):
            raise FlacError("read past the end")
        v = int.from_bytes(self.data[b0:b1], "big") >> (b1 * 8 - (p + n))
        self.pos = p + n
        return v & ((1 << n) - 1)

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v


_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
_SAMPLE_SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}


def _frame_header(data, pos, info):
    """the header at byte `pos`: (dict, bytes of the header including its CRC-8)"""
    r = _Bits(data, pos * 8)
    if r.u(14) != 0x3FFE:
        raise FlacError(f"no frame sync at byte {pos}")
    if r.u(1):
        raise FlacError("reserved bit set")
    variable = r.u(1)
    bs_code, sr_code, assign, ss_code = r.u(4), r.u(4), r.u(4), r.u(3)
    if r.u(1):
        raise FlacError("reserved bit set")
    lead = r.u(8)
    if lead < 0x80:
        number = lead
    else:
        extra = 0
        while lead & (0x40 >> extra):
            extra += 1
        if extra == 0 or extra > 6:
            raise FlacError("bad coded number")
        number = lead & ((1 << (6 - extra)) - 1)
        for _ in range(extra):
            c = r.u(8)
            if c >> 6 != 2:
                raise FlacError("bad continuation byte in the coded number")
            number = (number << 6) | (c & 63)
    if bs_code == 0:
        raise FlacError("reserved block size code")
    if bs_code == 1:
        bs = 192
    elif bs_code <= 5:
        bs = 576 << (bs_code - 2)
    elif bs_code == 6:
        bs = r.u(8) + 1
    elif bs_code == 7:
        bs = r.u(16) + 1
    else:
        bs = 256 << (bs_code - 8)
    if sr_code == 0:
        sr = info.get("samplerate") if info else None
    elif sr_code in _RATES:
        sr = _RATES[sr_code]
    elif sr_code == 12:
        sr = r.u(8) * 1000
    elif sr_code == 13:
        sr = r.u(16)
    elif sr_code == 14:
        sr = r.u(16) * 10
    else:
        raise FlacError("invalid sample rate code")
    if ss_code == 0:
        bps = info["bits_per_sample"] if info else None
    elif ss_code in _SAMPLE_SIZES:
        bps = _SAMPLE_SIZES[ss_code]
    else:
        raise FlacError("reserved sample size code")
    if assign > 10:
        raise FlacError("reserved channel assignment")
    n = r.pos // 8 - pos
    crc = r.u(8)
    if crc8(data[pos:pos + n]) != crc:
        raise FlacError(f"frame header CRC-8 mismatch at byte {pos}")
    return {"variable": variable, "blocksize": bs, "samplerate": sr, "assignment": assign, "channels": 2 if assign >= 8 else assign + 1,
            "bits_per_sample": bps, "number": number, "blocksize_code": bs_code, "samplerate_code": sr_code}, n + 1


def _gather(bits, first, n, width):
    """n unsigned fields of `width` bits starting at the positions `first` (an int array)"""
    if width == 0:
        return np.zeros(n, np.int64)
    idx = first[:, None] + np.arange(width)[None, :]
    return (bits[idx].astype(np.int64) << np.arange(width - 1, -1, -1)[None, :]).sum(1)


def _residual(r, bits, nxt, bs, order):
    """the coded residual of one subframe: (int64 [bs - order], partition order, method, parameters (None = escape))"""
    method = r.u(2)
    if method > 1:
        raise FlacError("reserved residual coding method")
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    po = r.u(4)
    if bs % (1 << po) or (bs >> po) < order or (po and (bs >> po) == 0):
        raise FlacError("partition order does not fit the block")
    out = np.empty(bs - order, np.int64)
    params, done = [], 0
    for j in range(1 << po):
        n = (bs >> po) - (order if j == 0 else 0)
        k = r.u(pbits)
        if k == esc:
            width = r.u(5)
            params.append(None)
            v = _gather(bits, r.pos + width * np.arange(n, dtype=np.int64), n, width)
            if width:
                v = np.where(v >> (width - 1), v - (1 << width), v)
            r.pos += n * width
        else:
            params.append(k)
            p = r.pos
            ends = [0] * n
            step = 1 + k
            for t in range(n):
                q = nxt[p]
                ends[t] = q
                p = q + step
            if n and ends[-1] >= len(nxt) - 1:
                raise FlacError("unary code runs past the end")
            e = np.asarray(ends, np.int64)
            starts = np.empty(n, np.int64)
            if n:
                starts[0] = r.pos
                starts[1:] = e[:-1] + step
            u = ((e - starts) << k) | _gather(bits, e + 1, n, k)
            v = (u >> 1) ^ -(u & 1)
            r.pos = p
        out[done:done + n] = v
        done += n
    return out, po, method, params


def _subframe(r, bits, nxt, bs, bps):
    if r.u(1):
        raise FlacError("subframe padding bit set")
    kind = r.u(6)
    wasted = 0
    if r.u(1):
        wasted = 1
        while not r.u(1):
            wasted += 1
    bps -= wasted
    sub = {"wasted": wasted, "bits": bps, "start": r.pos}
    if kind == 0:
        sub.update(type="CONSTANT", order=0, x=np.full(bs, r.s(bps), np.int64), coefs=[], shift=0)
    elif kind == 1:
        v = _gather(bits, r.pos + bps * np.arange(bs, dtype=np.int64), bs, bps)
        r.pos += bs * bps
        sub.update(type="VERBATIM", order=0, x=np.where(v >> (bps - 1), v - (1 << bps), v), coefs=[], shift=0)
    elif 8 <= kind <= 12 or kind >= 32:
        order = kind - 8 if kind < 32 else kind - 31
        if order > bs:
            raise FlacError("predictor order above the block size")
        x = np.zeros(bs, np.int64)
        for i in range(order):
            x[i] = r.s(bps)
        if kind < 32:
            coefs, shift, precision = _FIXED[order], 0, 0
        else:
            precision = r.u(4) + 1
            if precision == 16:
                raise FlacError("invalid coefficient precision")
            shift = r.s(5)
            if shift < 0:
                raise FlacError("negative predictor shift")
            coefs = [r.s(precision) for _ in range(order)]
        x[order:], po, method, params = _residual(r, bits, nxt, bs, order)
        sub.update(type="FIXED" if kind < 32 else "LPC", order=order, x=x, coefs=coefs, shift=shift, precision=precision,
                   partition_order=po, method=method, params=params)
    else:
        raise FlacError(f"reserved subframe type {kind}")
    return sub


def _restore(subs):
    """undo the predictors of all FIXED / LPC subframes in place: x[i] = residual[i] + (sum_j coef[j] x[i - 1 - j] >> shift), 64-bit"""
    groups = {}
    for s in subs:
        if s["order"]:
            groups.setdefault(len(s["x"]), []).append(s)
    for bs, group in groups.items():
        w = max(s["order"] for s in group)
        n = len(group)
        X = np.zeros((n, w + bs), np.int64)
        C = np.zeros((n, w), np.int64)
        order = np.empty(n, np.int64)
        shift = np.empty(n, np.int64)
        for i, s in enumerate(group):
            X[i, w:] = s["x"]
            C[i, w - s["order"]:] = s["coefs"][::-1]
            order[i], shift[i] = s["order"], s["shift"]
        for i in range(bs):
            pred = (C * X[:, i:i + w]).sum(1) >> shift
            X[:, w + i] += np.where(order <= i, pred, 0)
        for i, s in enumerate(group):
            s["x"] = X[i, w:].copy()


def decode_frames(data: bytes, info=None, offset=0, max_frames=None):
    """Decode audio frames from byte `offset` to the end of `data` (or `max_frames` of them).  Every CRC is verified.
    Returns (int64 [n, channels], [frame dict: offset, size, blocksize, assignment, number, bits_per_sample, subframes])."""
    frames, subs = [], []
    pos, end = offset, len(data)
    while pos < end and (max_frames is None or len(frames) < max_frames):
        h, hlen = _frame_header(data, pos, info)
        bs, bps, nch = h["blocksize"], h["bits_per_sample"], h["channels"]
        bound = (info or {}).get("max_framesize") or 0
        if not bound:
            bound = 2 * (32 + nch * (bps + 2) * bs // 8)
        window = np.frombuffer(data, np.uint8, min(bound + 8, end - pos), pos)
        bits = np.unpackbits(window)
        idx = np.where(bits, np.arange(len(bits), dtype=np.int64), len(bits))
        nxt = np.append(np.minimum.accumulate(idx[::-1])[::-1], len(bits)).tolist()
        bits = np.append(bits, np.zeros(64, np.uint8))
        r = _Bits(bytes(window), hlen * 8)
        fs = []
        for c in range(nch):
            side = (h["assignment"] == 8 and c == 1) or (h["assignment"] == 9 and c == 0) or (h["assignment"] == 10 and c == 1)
            fs.append(_subframe(r, bits, nxt, bs, bps + (1 if side else 0)))
        r.pos = (r.pos + 7) // 8 * 8
        size = r.pos // 8 + 2
        if size > len(window):
            raise FlacError("frame runs past the end")
        if crc16(window[:size - 2].tobytes()) != r.u(16):
            raise FlacError(f"frame CRC-16 mismatch in the frame at byte {pos}")
        h.update(offset=pos, size=size, subframes=fs)
        frames.append(h)
        subs.extend(fs)
        pos += size
    _restore(subs)
    out = []
    for h in frames:
        ch = [s["x"] << s["wasted"] for s in h["subframes"]]
        a = h["assignment"]
        if a == 8:
            ch[1] = ch[0] - ch[1]
        elif a == 9:
            ch[0] = ch[0] + ch[1]
        elif a == 10:
            mid = (ch[0] << 1) | (ch[1] & 1)
            ch[0], ch[1] = (mid + ch[1]) >> 1, (mid - ch[1]) >> 1
        out.append(np.stack(ch, 1))
        for s in h["subframes"]:
            del s["x"]
    pcm = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return pcm, frames


def decode(data: bytes, max_frames=None):
    """A whole .flac file: (STREAMINFO dict, int64 PCM [n, channels], frames)"""
    info, _, first = parse_container(data)
    pcm, frames = decode_frames(data, info, first, max_frames)
    return info, pcm, frames


def pcm_bytes(pcm, bits_per_sample) -> bytes:
    """little-endian interleaved PCM at the stream's sample width: what STREAMINFO's MD5 is taken over"""
    nbytes = (bits_per_sample + 7) // 8
    a = np.ascontiguousarray(pcm, np.int64).reshape(-1)
    if nbytes == 2:
        return a.astype("<i2").tobytes()
    if nbytes == 4:
        return a.astype("<i4").tobytes()
    u = (a & ((1 << (8 * nbytes)) - 1)).astype(np.uint64)
    return np.stack([(u >> (8 * i)) & 255 for i in range(nbytes)], 1).astype(np.uint8).tobytes()


# ---- exact size of a fixed-predictors-only encoding -------------------------------------------------------------------------
def _max_partition_order(bs, order):
    mp = 0
    while mp < 6 and (bs >> mp) % 2 == 0:
        mp += 1
    while mp > 0 and (bs >> mp) <= order:
        mp -= 1
    return mp


def _fixed_subframe_bits(x, bps):
    """x int64 [nb, bs]: bits per block of the cheapest of CONSTANT, VERBATIM and FIXED orders 0..4 with Rice method 0, parameters
    0..14 and partition orders 0..6 (those that divide the block and leave the first partition non-empty), no escapes"""
    nb, bs = x.shape
    best = np.where((x == x[:, :1]).all(1), 8 + bps, 8 + bps * bs).astype(np.int64)
    for order in range(0, 5):
        if order >= bs:
            break
        r = np.diff(x, n=order, axis=1) if order else x
        u = (r << 1) ^ (r >> 63)
        mp = _max_partition_order(bs, order)
        F = 1 << mp
        fine = np.empty((15, nb, F), np.int64)
        pad = np.zeros((nb, order), np.int64)
        for k in range(15):
            fine[k] = np.concatenate([pad, u >> k], 1).reshape(nb, F, bs // F).sum(2)
        cost = None
        for po in range(mp + 1):
            parts = fine.reshape(15, nb, 1 << po, F >> po).sum(3)
            n = np.full(1 << po, bs >> po, np.int64)
            n[0] -= order
            parts = parts + (np.arange(1, 16)[:, None, None] * n[None, None, :])
            c = (parts.min(0) + 4).sum(1)
            cost = c if cost is None else np.minimum(cost, c)
        best = np.minimum(best, 8 + order * bps + 2 + 4 + cost)
    return best


def _header_bytes(number, bs, nominal, samplerate):
    n = 4 + 1
    n += 1 if number < 0x80 else 2 if number < 0x800 else 3 if number < 0x10000 else 4 if number < 0x200000 else 5 if number < 0x4000000 else 6
    if bs != nominal or bs not in (192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768):
        n += 1 if bs <= 256 else 2
    if samplerate not in _RATES.values():
        n += 2
    return n


def fixed_only_bytes(pcm, block_size, samplerate=44100) -> int:
    """Exact audio-frame bytes of a 16-bit stereo stream coded at `block_size` with fixed predictors only: per channel the cheapest
    of CONSTANT, VERBATIM and FIXED orders 0..4, per frame the cheapest of the four stereo modes, headers, padding and CRCs included."""
    a = np.asarray(pcm, np.int64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("fixed_only_bytes expects [n, 2]")
    n = a.shape[0]
    full = n // block_size
    total, number = 0, 0
    for lo, hi, bs in ((0, full * block_size, block_size), (full * block_size, n, n - full * block_size)):
        if hi == lo:
            continue
        l, r = a[lo:hi, 0].reshape(-1, bs), a[lo:hi, 1].reshape(-1, bs)
        b = {"l": _fixed_subframe_bits(l, 16), "r": _fixed_subframe_bits(r, 16), "m": _fixed_subframe_bits((l + r) >> 1, 16),
             "s": _fixed_subframe_bits(l - r, 17)}
        bits = np.minimum(np.minimum(b["l"] + b["r"], b["l"] + b["s"]), np.minimum(b["s"] + b["r"], b["m"] + b["s"]))
        for v in bits:
            total += _header_bytes(number, bs, block_size, samplerate) + (int(v) + 7) // 8 + 2
            number += 1
    return total
