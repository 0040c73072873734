"""The host side of FLAC input files (audio_io.flac_stream, audio_io.is_flac, the loader's refusal), without a GPU."""
import os

import pytest

from audio_separator_amd import audio_io
from tests import flac_ref as F
from tests import flac_synth as Y

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac")
KEYS = ("min_blocksize", "max_blocksize", "min_framesize", "max_framesize", "samplerate", "channels", "bits_per_sample", "total_samples", "md5")


@pytest.mark.parametrize("name", sorted(os.listdir(FIX)))
def test_flac_stream_reads_the_fixtures(name):
    path = os.path.join(FIX, name)
    with open(path, "rb") as f:
        data = f.read()
    info, _, first = F.parse_container(data)
    got = audio_io.flac_stream(path)
    assert {k: got[k] for k in KEYS} == info
    assert (got["audio_offset"], got["audio_bytes"]) == (first, len(data) - first) and audio_io.is_flac(path)
    assert audio_io.flac_info(path)["bits"] == got["bits_per_sample"]             # the older probe is unchanged


@pytest.mark.parametrize("name", ["id3v2_prefix", "metadata_blocks", "total_samples_0", "trailing_tag", "mono", "bits_24"])
def test_flac_stream_reads_the_containers(tmp_path, name):
    s = Y.streams()[name]
    path = str(tmp_path / "x.bin")                                                # found by the marker, not by the extension
    with open(path, "wb") as f:
        f.write(s["file"])
    got = audio_io.flac_stream(path)
    assert {k: got[k] for k in KEYS} == s["info"] and audio_io.is_flac(path)
    assert (got["audio_offset"], got["audio_bytes"]) == (s["audio_offset"], s["audio_bytes"])


def test_what_is_not_flac(tmp_path):
    for i, blob in enumerate((b"", b"RIFF" + bytes(40), b"ID3\x04\x00\x00\x00\x00\x00\x10" + bytes(16) + b"RIFF", b"fLaC", b"fLaC\x81\x00\x00\x22" + bytes(34),
                              b"fLaC\x00\x00\x00\x22" + bytes(34) + b"\x81\x00\x10\x00")):
        path = str(tmp_path / f"{i}.flac")
        with open(path, "wb") as f:
            f.write(blob)
        with pytest.raises(audio_io.AudioIOError):
            audio_io.flac_stream(path)
    assert not audio_io.is_flac(str(tmp_path / "0.flac")) and not audio_io.is_flac(str(tmp_path / "1.flac"))
    assert not audio_io.is_flac(str(tmp_path / "missing.flac"))


def test_loader_says_where_flac_is_decoded(tmp_path):
    if audio_io._optional("librosa") is not None:
        pytest.skip("librosa is installed: it decodes the file")
    path = str(tmp_path / "song.flac")
    with open(path, "wb") as f:
        f.write(Y.streams()["verbatim"]["file"])
    with pytest.raises(audio_io.AudioIOError, match="decoded on the device") as e:
        audio_io.load(path, sr=44100)
    assert path in str(e.value)
    with open(path, "wb") as f:
        f.write(Y.streams()["rate_code_12_32000"]["file"])
    with pytest.raises(audio_io.AudioIOError, match="is sampled at 32000 Hz"):
        audio_io.load(path, sr=44100)
    other = str(tmp_path / "song.ogg")
    with open(other, "wb") as f:
        f.write(b"OggS" + bytes(60))
    with pytest.raises(audio_io.AudioIOError, match="install librosa") as e:      # other containers keep their text
        audio_io.load(other, sr=44100)
    assert "decoded on the device" not in str(e.value)
