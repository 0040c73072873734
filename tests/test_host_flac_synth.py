"""Every stream of tests/flac_synth.py, pinned on the CPU to the independent decoder tests/flac_ref.py: it decodes without error to the
samples the description stands for.  This is what qualifies the streams as inputs of the device decoder's tests."""
import numpy as np
import pytest

from tests import flac_ref as F
from tests import flac_synth as Y

NAMES = sorted(Y.streams())


def test_the_list_covers_what_the_decoder_must_take():
    have = set(NAMES)
    for bs in (16, 17, 255, 257, 4097, 192, 576, 4608, 256, 4096, 16384):
        assert f"block_{bs}" in have
    for bits in (8, 12, 16, 20, 24):
        assert {f"bits_{bits}", f"bits_{bits}_streaminfo"} <= have
    assert {"constant", "verbatim", "fixed_orders", "lpc_orders", "lpc_sum_over_32_bits", "rice0_k0_k14", "rice1_k30", "escapes_0_1_25",
            "partition_max", "partition_first_empty", "long_unary_run", "wasted_bits", "wasted_bits_side", "assignments_16", "assignments_24",
            "mono", "variable_blocks", "short_last_frame", "frame_inside_verbatim", "id3v2_prefix", "metadata_blocks", "total_samples_0",
            "trailing_tag"} <= have
    assert {f"damaged_{how}_{j}" for how in ("body", "header", "cut") for j in (0, 2, 3)} <= have
    assert {n.split("_")[2] for n in have if n.startswith("rate_code_")} == {"0", "12", "13", "14"}


@pytest.mark.parametrize("name", NAMES)
def test_stream_decodes_to_its_description(name):
    s = Y.streams()[name]
    data = s["file"][s["marker_offset"]:]
    info, blocks, first = F.parse_container(data)
    assert first + s["marker_offset"] == s["audio_offset"] and info == s["info"]
    pcm, frames = F.decode_frames(data, info, first, max_frames=s["n_frames"])
    assert len(frames) == s["n_frames"]
    assert np.array_equal(pcm.reshape(len(pcm), -1), s["pcm"].reshape(len(s["pcm"]), -1)) if s["n_frames"] else len(pcm) == 0
    assert [f["offset"] - first for f in frames] == s["frame_offsets"][:s["n_frames"]]
    assert (frames[-1]["offset"] + frames[-1]["size"] - first if frames else 0) == s["bytes_consumed"]
    if s["bytes_consumed"] < s["audio_bytes"]:            # a damaged frame or a tag follows: the reference refuses to go on
        with pytest.raises((F.FlacError, IndexError)):    # (IndexError: its unary walk on a frame that is cut)
            F.decode_frames(data, info, first + s["bytes_consumed"], max_frames=1)


def test_the_descriptions_reach_the_corners():
    """what the stream names promise, read back from flac_ref's parse"""
    S = Y.streams()

    def subs(name):
        s = S[name]
        data = s["file"][s["marker_offset"]:]
        info, _, first = F.parse_container(data)
        return [sf for f in F.decode_frames(data, info, first, max_frames=s["n_frames"])[1] for sf in f["subframes"]], s
    lpc, _ = subs("lpc_orders")
    assert {(x["order"], x["precision"], x["shift"]) for x in lpc} >= {(1, 1, 0), (1, 15, 15), (8, 15, 0), (12, 15, 14), (32, 15, 15), (32, 1, 0)}
    esc, _ = subs("escapes_0_1_25")
    assert esc[0]["params"][:3] == [None, None, None] and esc[1]["method"] == 1
    pm, _ = subs("partition_max")
    assert pm[0]["partition_order"] == 12 and pm[1]["partition_order"] == 0
    pe, _ = subs("partition_first_empty")
    assert all((64 >> x["partition_order"]) == x["order"] for x in pe)
    r1, _ = subs("rice1_k30")
    assert r1[0]["method"] == 1 and r1[0]["params"] == [30]
    r0, _ = subs("rice0_k0_k14")
    assert r0[0]["params"] == [0] and r0[1]["params"] == [14]
    w, _ = subs("wasted_bits")
    assert sorted(x["wasted"] for x in w) == [1, 7, 8, 8]
    ws, _ = subs("wasted_bits_side")
    assert ws[1]["wasted"] == 1 and ws[1]["bits"] == 16
    s = S["long_unary_run"]
    assert s["info"]["max_framesize"] > 4096 // 8 * 2
    s = S["frame_inside_verbatim"]
    a = Y.audio(s)
    inner = s["frame_offsets"][1] + 7
    h, hlen = F._frame_header(a, inner, s["info"])                       # a complete header with a valid CRC-8 ...
    _, fr = F.decode_frames(a, s["info"], inner, max_frames=1)           # ... and a frame whose CRC-16 holds
    assert h["blocksize"] == 192 and fr[0]["size"] == 14 and inner + 14 < s["frame_offsets"][2]
    v = S["variable_blocks"]
    assert v["info"]["min_blocksize"] == 16 and v["info"]["max_blocksize"] == 4097
    assert S["total_samples_0"]["info"]["total_samples"] == 0 and S["max_framesize_0"]["info"]["max_framesize"] == 0
    assert S["id3v2_prefix"]["marker_offset"] == 182 and S["trailing_tag"]["audio_bytes"] - S["trailing_tag"]["bytes_consumed"] == 128
