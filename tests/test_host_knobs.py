"""The environment knobs of libasx.so (csrc/knobs.h) compiled for the HOST (g++) by tests/host/knobs_host.cpp, in the default and the
experimental build: every knob, set to each value of VALUES one at a time, must give every field the value of the expression the library
used at its read site before the knobs moved into one table (transcribed below).  The same file checks two claims about the sources:
getenv is called in knobs.h only, and no kernel-attribute guard of the unlocked "once" kinds is left beside a hipFuncSetAttribute."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-audio-separator_amd", "csrc")
VALUES = [None, "", "0", "1", "-3", "7", "200", "abc"]       # None: unset


def atoi(v):
    m = re.match(r"\s*([+-]?\d+)", v)
    return int(m.group(1)) if m else 0


def atof(v):
    m = re.match(r"\s*([+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?)", v)
    return float(m.group(1)) if m else 0.0


# field -> (variable, value for v, the variable's value or None), one line per read site of the parent sources
KNOBS = {
    # engine_core.h
    "poison": ("ASX_POISON", lambda v: atoi(v) if v is not None else -1),
    "fft_radix4": ("ASX_FFT_RADIX4", lambda v: v is not None and atoi(v) != 0),
    # asx.hip
    "finalize4": ("ASX_FINALIZE4", lambda v: not (v is not None and atoi(v) == 0)),
    "prof_dump": ("ASX_PROF_DUMP", lambda v: v is not None),
    # engine_mdx.h
    "up_nrep": ("ASX_UP_NREP", lambda v: atoi(v) if v is not None else 0),
    "conv_kc4": ("ASX_CONV_KC4", lambda v: atoi(v) if v is not None else 1 << 30),
    "conv_kc4_n2": ("ASX_CONV_KC4_N2", lambda v: atoi(v) if v is not None else 1),
    "down_kc2": ("ASX_DOWN_KC2", lambda v: atoi(v) if v is not None else 1),
    "down6_wide": ("ASX_DOWN6_WIDE", lambda v: atoi(v) if v is not None else 1),
    "nt": ("ASX_NT", lambda v: atoi(v) if v is not None else 0),
    "no_dma": ("ASX_NO_DMA", lambda v: v is not None),
    "winos_abl": ("ASX_WINOS_ABL", lambda v: atoi(v) if v is not None else 0),
    "wino_abl": ("ASX_WINO_ABL", lambda v: atoi(v) if v is not None else 0),
    "wino_cfg": ("ASX_WINO_CFG", lambda v: atoi(v) if v is not None else 6),
    "gemm_bk64": ("ASX_GEMM_BK64", lambda v: v is not None),
    "tdf2": ("ASX_TDF2", lambda v: atoi(v) if v is not None else 1),          # ASX_TDF2_DEFAULT
    "tdf2_sbit": ("ASX_TDF2_SBIT", lambda v: atoi(v) if v is not None else 8),
    "tdf2_abl": ("ASX_TDF2_ABL", lambda v: atoi(v) if v is not None else 0),
    "tdf2_bk16": ("ASX_TDF2_BK16", lambda v: atoi(v) if v is not None else 0),
    "tdf3_map": ("ASX_TDF3_MAP", lambda v: atoi(v) if v is not None else -1),
    "tdf3_nw8": ("ASX_TDF3_NW8", lambda v: not (v is not None and atoi(v) == 0)),
    "tdf3_abl": ("ASX_TDF3_ABL", lambda v: atoi(v) if v is not None else 0),
    "tdf3_abl_set": ("ASX_TDF3_ABL", lambda v: v is not None),
    "f16x3_n": ("ASX_F16X3_N", lambda v: atoi(v) if v is not None else 0),
    "f16x3_n_set": ("ASX_F16X3_N", lambda v: v is not None),
    "gemm_t128": ("ASX_GEMM_T128", lambda v: atoi(v) if v is not None else 1),
    "tdf2_small": ("ASX_TDF2_SMALL", lambda v: atoi(v) if v is not None else 0),
    "tdf3_eff128": ("ASX_TDF3_EFF128", lambda v: atof(v) if v is not None else 0.96),
    "tdf3_eff128_set": ("ASX_TDF3_EFF128", lambda v: v is not None),
    "fft3_gs": ("ASX_FFT3_GS", lambda v: max(1, atoi(v)) if v is not None else 16),
    "fft3_g": ("ASX_FFT3_G", lambda v: max(5, atoi(v)) if v is not None else 16),
    "istft_abl": ("ASX_ISTFT_ABL", lambda v: atoi(v) if v is not None else 0),
    "tdf_inplace": ("ASX_TDF_INPLACE", lambda v: v is not None and atoi(v) != 0),
    # engine_hd.h (HD_MAX_GROUPS = 6)
    "hd_mha_db": ("ASX_MHA_DB", lambda v: not (v is not None and atoi(v) == 0)),
    "hd_groups": ("ASX_HD_GROUPS", lambda v: max(1, min(6, atoi(v))) if v is not None else 6),
    # engine_ht.h
    "halo": ("ASX_HALO", lambda v: not (v is not None and atoi(v) == 0)),     # was `off = set && atoi == 0`
    "gg_lowai": ("ASX_GG_LOWAI", lambda v: atof(v) if v is not None else 90.0),
    "gg_smallgrid": ("ASX_GG_SMALLGRID", lambda v: atoi(v) if v is not None else 1024),
    "gather6": ("ASX_GATHER6", lambda v: not (v is not None and atoi(v) == 0)),
    "gather6_minn": ("ASX_GATHER6_MINN", lambda v: atoi(v) if v is not None else 48),
    "gather6_glu": ("ASX_GATHER6_GLU", lambda v: not (v is not None and atoi(v) == 0)),
    "gather6_strided": ("ASX_GATHER6_STRIDED", lambda v: not (v is not None and atoi(v) == 0)),
    "gather6_partial": ("ASX_GATHER6_PARTIAL", lambda v: not (v is not None and atoi(v) == 0)),
    "halo_minblk": ("ASX_HALO_MINBLK", lambda v: atoi(v) if v is not None else 0),
    "ht_linear_small": ("ASX_HT_LINEAR_SMALL", lambda v: not (v is not None and atoi(v) == 0)),
    "ht_mha_db": ("ASX_MHA_DB", lambda v: v is not None and atoi(v) != 0),
    "mha6": ("ASX_MHA6", lambda v: not (v is not None and atoi(v) == 0)),
    "attn_exact": ("ASX_ATTN_EXACT", lambda v: int(v is not None)),
    # engine_rof.h
    "rof_normfuse": ("ASX_ROF_NORMFUSE", lambda v: not (v is not None and atoi(v) == 0)),
    "rof_gelu": ("ASX_ROF_GELU", lambda v: atoi(v) if v is not None else 2),
    "attn_db": ("ASX_ATTN_DB", lambda v: v is not None and atoi(v) != 0),
    "attn_qw": ("ASX_ATTN_QW", lambda v: atoi(v) if v is not None else 1),
    "attn6": ("ASX_ATTN6", lambda v: not (v is not None and atoi(v) == 0)),
    "attn6_qw": ("ASX_ATTN6_QW", lambda v: atoi(v) if v is not None else 2),
    "rof_fuse": ("ASX_ROF_FUSE", lambda v: not (v is not None and atoi(v) == 0)),
    "attn_v1": ("ASX_ATTN_V1", lambda v: v is not None and atoi(v) != 0),
    # kernels_halo.h, kernels_ht.h
    "halo_nt": ("ASX_HALO_NT", lambda v: atoi(v) if v is not None else 0),
    "halo_split128": ("ASX_HALO_SPLIT128", lambda v: v is not None and atoi(v) != 0),
    "gg_legacy": ("ASX_GG_LEGACY", lambda v: v is not None),
    "gg_m128": ("ASX_GG_M128", lambda v: not (v is not None and atoi(v) == 0)),
    # per engine: the asx_engine member initialisers of engine_core.h, ASX_FFT3 / ASX_FFT3P of asx_engine_create
    "gemm_bf16x6": ("ASX_GEMM_BF16X6", lambda v: atoi(v) if v is not None else 1),
    "gemm_f16x3": ("ASX_GEMM_F16X3", lambda v: atoi(v) if v is not None else 1),
    "wino6": ("ASX_WINO6", lambda v: max(0, atoi(v)) if v is not None else 144),
    "conv3h": ("ASX_CONV3H", lambda v: max(0, atoi(v)) if v is not None else 144),
    "down6": ("ASX_DOWN6", lambda v: atoi(v) if v is not None else 1),
    "up6": ("ASX_UP6", lambda v: atoi(v) if v is not None else 1),
    "fft3": ("ASX_FFT3", lambda v: not (v is not None and atoi(v) == 0)),
    "fft3p": ("ASX_FFT3P", lambda v: not (v is not None and atoi(v) == 0)),
}
# the knobs whose rule depends on the build
EXPERIMENTAL = {
    "winograd": ("ASX_WINOGRAD", lambda v: max(0, atoi(v)) if v is not None else 3),
    "winos": ("ASX_WINOS", lambda v: max(0, atoi(v)) if v is not None else 0),
    "pair_images": ("ASX_PAIR_IMAGES", lambda v: atoi(v) if v is not None else 0),
}
DEFAULT_BUILD = {
    "winograd": ("ASX_WINOGRAD", lambda v: (0 if atoi(v) <= 0 else 3) if v is not None else 3),
    "winos": ("ASX_WINOS", lambda v: 0),
    "pair_images": ("ASX_PAIR_IMAGES", lambda v: 0),
}


@pytest.fixture(scope="module", params=[False, True], ids=["default", "experimental"])
def build(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knobs") / "knobs_host")
    flags = ["-DASX_EXPERIMENTAL_KERNELS"] if request.param else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "knobs_host.cpp")],
                   check=True)
    return exe, dict(KNOBS, **(EXPERIMENTAL if request.param else DEFAULT_BUILD))


def run(exe, scenarios):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASX_")}
    out = subprocess.run([exe] + scenarios, env=env, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(scenarios)
    return [dict(f.split("=") for f in line.split()) for line in out]


def test_table_lists_every_knob_of_the_header(build):
    _, table = build
    src = open(os.path.join(CSRC, "knobs.h")).read()
    assert {name for name, _ in table.values()} == set(re.findall(r'"(ASX_[A-Z0-9_]+)"', src))
    assert len({name for name, _ in table.values()}) == 67


def test_every_knob_reads_as_before(build):
    exe, table = build
    names = sorted({name for name, _ in table.values()})
    scenarios = [name if v is None else f"{name}={v}" for name in names for v in VALUES]
    got = run(exe, scenarios)
    assert set(got[0]) == set(table), "knobs_host prints a field the table does not transcribe, or misses one"
    bad = []
    for sc, fields in zip(scenarios, got):
        name, _, val = sc.partition("=")
        val = val if "=" in sc else None
        for field, (var, rule) in table.items():
            want = rule(val if var == name else None)
            if float(fields[field]) != float(want):         # bools print as 0 / 1, doubles as %.17g (exact)
                bad.append(f"{sc}: {field} = {fields[field]}, expected {want}")
    assert not bad, "\n".join(bad[:20])


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hip")):
            yield f, open(os.path.join(CSRC, f)).read()


def test_getenv_only_in_knobs_header():
    assert [f for f, src in _sources() if "getenv(" in src and f != "knobs.h"] == []


def test_no_unlocked_attribute_guards():
    """Every guarded LDS grant goes through grant_lds (asx.hip); what stays beside a hipFuncSetAttribute call are the unconditional
    ones of load time."""
    guard = re.compile(r"static\s+(const\s+)?(bool|int)\s+\w+\s*=|std::set\s*<")
    bad = []
    for f, src in _sources():
        lines = src.splitlines()
        for i, line in enumerate(lines):
            if "hipFuncSetAttribute" in line:
                bad += [f"{f}:{j + 1}" for j in range(max(0, i - 8), i) if guard.search(lines[j])]
    assert bad == []
