"""Host side of the MDXC norm / act variants (no GPU): the YAML norm / act parser against the reference's get_norm / get_act
verdicts (tests/golden/mdxc_variants.npz, written by make_golden_mdxc_variants.py), the BatchNorm fold of csrc/v3_norm.h
against F.batch_norm in float64, the split rule of the GroupNorm statistics pass, and the header's list of accepted kinds."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mdxc_variants.npz")


@pytest.fixture(scope="module")
def E():
    from audio_separator_amd import engine
    return engine


@pytest.fixture(scope="module")
def table():
    return json.loads(str(np.load(GOLDEN)["parser_table"]))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("v3norm") / "v3_norm_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "v3_norm_host.cpp")], check=True)
    return exe


def test_norm_parser_matches_reference(E, table):
    kinds = {"Identity": E.V3_NORM_NONE, "BatchNorm2d": E.V3_NORM_BATCH, "InstanceNorm2d": E.V3_NORM_INSTANCE}
    assert len(table["norm"]) >= 10
    for row in table["norm"]:
        if row["kind"] == "error":
            with pytest.raises(ValueError):
                E.v3_norm_act_codes(row["s"], "gelu")
            continue
        want = E.V3_NORM_GROUP + row["groups"] if row["kind"] == "GroupNorm" else kinds[row["kind"]]
        assert E.v3_norm_act_codes(row["s"], "gelu")[0] == want, row


def test_act_parser_matches_reference(E, table):
    kinds = {"GELU": E.V3_ACT_GELU, "ReLU": E.V3_ACT_RELU, "ELU": E.V3_ACT_ELU}
    assert len(table["act"]) >= 10
    for row in table["act"]:
        if row["kind"] == "error":
            with pytest.raises(ValueError):
                E.v3_norm_act_codes(None, row["s"])
            continue
        _, a, alpha = E.v3_norm_act_codes(None, row["s"])
        assert a == kinds[row["kind"]], row
        if row["kind"] == "ELU":
            assert alpha == row["alpha"], row


def test_bn_fold_equals_batch_norm_eval(host_exe, tmp_path):
    c = 48
    rng = np.random.default_rng(7)
    w = rng.uniform(0.5, 1.5, c).astype(np.float32)
    b = (0.2 * rng.standard_normal(c)).astype(np.float32)
    m = rng.uniform(-0.3, 0.3, c).astype(np.float32)
    v = rng.uniform(0.5, 2.0, c).astype(np.float32)
    v[0] = 1e-7                                                    # eps dominates the denominator
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([w, b, m, v]).tofile(fin)
    subprocess.run([host_exe, "fold", str(c), str(fin), str(fout)], check=True)
    out = np.fromfile(fout, np.float32)
    scale, shift = out[:c].astype(np.float64), out[c:].astype(np.float64)
    x = torch.from_numpy(rng.standard_normal((3, c, 5, 7)))
    t = lambda a: torch.from_numpy(a.astype(np.float64))  # noqa: E731
    ref = F.batch_norm(x, t(m), t(v), t(w), t(b), training=False, eps=1e-5)
    got = x * torch.from_numpy(scale)[:, None, None] + torch.from_numpy(shift)[:, None, None]
    # scale and shift are float64 folds rounded once to float32: at most half an ulp each
    bound = 2.0 ** -24 * ((x * torch.from_numpy(scale)[:, None, None]).abs() + torch.from_numpy(shift).abs()[:, None, None]) * 1.01
    assert bool(((got - ref).abs() <= bound).all()), ((got - ref).abs() / bound).max()


def test_gn_split_rule(host_exe):
    def splits(B, G, n):
        return int(subprocess.run([host_exe, "splits", str(B), str(G), str(n)], check=True, capture_output=True, text=True).stdout)
    # the level-0 GroupNorm2 of tests/test_gpu_mdxc_variants.py::test_groupnorm_split_reduction_float64 (8 channels,
    # dim_t 256 x dim_f 1024 / 2 subbands): many slices per group
    assert splits(1, 2, 4 * 256 * 512) > 1
    assert splits(1, 2, 100) == 1                                 # short groups: one slice
    assert splits(64, 64, 1 << 30) >= 1 and splits(1, 1, 1 << 40) == 1024


def test_header_names_every_accepted_kind():
    with open(os.path.join(ROOT, "include", "asx.h")) as f:
        h = f.read()
    block = h[h.index("MDXC / TFC-TDF v3"):h.index("typedef struct asx_v3_config")]
    for word in ("None", "Identity", "InstanceNorm", "BatchNorm", "GroupNorm", "256 + G", "running_mean", "running_var",
                 "relu", "gelu", "elu", "__act_alpha__"):
        assert word in block, word
    assert re.search(r"0\s*=\s*relu,\s*1\s*=\s*gelu,\s*2\s*=\s*elu", block)
