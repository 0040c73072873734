"""The C ABI of invert_stem on device arrays (asx_invert_stem_dev, asx_invert_stem_batch_dev) as far as it can be checked without a
GPU, and the MDX plugin's ``invert_using_spec`` over the engine double, which must keep taking the host path."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from audio_separator_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("asx_invert_stem_dev", "asx_invert_stem_batch_dev")


@pytest.fixture(scope="module")
def lib():
    return E.load_library()


def test_symbols_declared_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "asx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(asx_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in E.SYMBOLS, name
        assert getattr(lib, name) is not None
    assert len(E.SYMBOLS) == len(set(E.SYMBOLS))
    assert lib.asx_abi_version() == E.ABI_VERSION == 8          # additive within ABI 7; ABI 8 added the STFT hooks


def test_song_struct_matches_the_header():
    """the ctypes mirror of asx_invert_song: the header's fields in the header's order"""
    hdr = open(os.path.join(ROOT, "include", "asx.h")).read()
    body = re.search(r"typedef struct asx_invert_song \{(.*?)\} asx_invert_song;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [n for n, _ in E._InvertSong._fields_] == ["mix_dev", "stem_dev", "out_dev", "n_samples", "out_capacity", "n_out",
                                                               "stem_layout"]
    assert C.sizeof(E._InvertSong) == 56                         # 3 pointers, 3 int64, one int32 and its padding


def test_song_struct_has_the_size_and_offsets_the_compiler_gives(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("gcc not available: the struct was not compiled")
    src ='#include <stdio.h>\n#include <stddef.h>\n#include "asx.h"\nint main(void) {\n' \
          '  printf("%zu %zu %zu\\n", sizeof(asx_invert_song), offsetof(asx_invert_song, n_out), offsetof(asx_invert_song, stem_layout));\n' \
          "  return 0;\n}\n"
    c = tmp_path / "song.c"
    c.write_text(src)
    exe = tmp_path / "song"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)],
                   check=True)
    size, off_n_out, off_layout = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(E._InvertSong)
    assert off_n_out == E._InvertSong.n_out.offset and off_layout == E._InvertSong.stem_layout.offset


def test_null_engine_is_an_error_not_a_crash(lib):
    n_out = C.c_int64(-1)
    assert lib.asx_invert_stem_dev(None, None, None, 2048, 0, 1.0, None, 2048, C.byref(n_out), None) != 0
    assert b"asx_invert_stem_dev" in lib.asx_last_error() and n_out.value == -1
    songs = (E._InvertSong * 1)()
    songs[0].n_samples, songs[0].n_out = 2048, -1
    assert lib.asx_invert_stem_batch_dev(None, songs, 1, 1.0, None) != 0
    assert b"asx_invert_stem_batch_dev" in lib.asx_last_error() and songs[0].n_out == -1
    assert lib.asx_invert_stem_batch_dev(None, None, 0, 1.0, None) != 0


def test_plugin_over_the_engine_double_decodes_on_the_host(tmp_path, monkeypatch):
    """Without the device decoder (the double has none) ``invert_using_spec`` runs as before: host decode, MDXDemixer.separate_stems,
    host stems; ``stems_dev`` has nothing to leave on a device."""
    from tests import fake_engine
    from tests import separate_cases as SC
    fake_engine.install(monkeypatch)
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    _, cls, common, arch, wav, _ = SC.cases("mdx", str(tmp_path))[0]
    inst = SC.plugin_class(cls)(common_config=dict(common, invert_using_spec=True), arch_config=arch)
    assert type(inst.engine).__name__ == "OracleEngine" and not inst._fast_file_path_enabled()
    calls = []
    real = inst._dm.separate_stems
    monkeypatch.setattr(inst._dm, "separate_stems", lambda mix: calls.append(type(mix)) or real(mix))
    assert inst._device_decode(wav) is None
    names = inst.separate(wav, None)
    assert calls == [np.ndarray] and len(names) == 2
    assert isinstance(inst.primary_source, np.ndarray) and inst.primary_source.shape == (3000, 2)
    assert isinstance(inst.secondary_source, np.ndarray) and inst.secondary_source.shape == (2048, 2)
    assert inst._dev_stems == {}
    for n in names:
        assert os.path.isfile(os.path.join(common["output_dir"], n)), n
    inst.clear_file_specific_paths()
    assert inst.stems_dev(wav) is None
    many = []
    real_many = inst._dm.separate_stems_many
    monkeypatch.setattr(inst._dm, "separate_stems_many", lambda mixes: many.append(len(mixes)) or real_many(mixes))
    assert inst.separate_many([wav, wav]) == [names, names] and many == [2]
