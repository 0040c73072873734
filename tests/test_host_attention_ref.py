"""The float64 attention references of tests/test_gpu_attention.py (tests/attention_ref.py), checked without a GPU: the plain
form against torch's scaled_dot_product_attention, the gated Roformer form against a transcription of the sequence walk of
oracle/roformer_oracle.py:_attention, the LocalState form against the score formula of oracle/hdemucs_oracle._local_state; and
the two mutants the GPU test uses to show its bars can catch a wrong kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as R


@pytest.mark.parametrize("nq,nk,heads,dh", [(1, 1, 1, 48), (65, 129, 2, 64), (100, 37, 3, 48), (130, 130, 2, 16)])
def test_plain_matches_sdpa(nq, nk, heads, dh):
    rng = np.random.default_rng(nq * 1000 + nk)
    B = 2
    q = rng.standard_normal((B * nq, heads * dh + 4))     # padded rows: only heads * dh columns are read
    k = rng.standard_normal((B * nk, heads * dh))
    v = rng.standard_normal((B * nk, heads * dh + 8))
    got = R.mha(q, k, v, B, nq, nk, heads, dh)

    def th(x, n):
        return torch.from_numpy(x[:, :heads * dh]).reshape(B, n, heads, dh).transpose(1, 2)
    ref = F.scaled_dot_product_attention(th(q, nq), th(k, nk), th(v, nk)).transpose(1, 2).reshape(B * nq, heads * dh)
    np.testing.assert_allclose(got, ref.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("axis,B,T,Fb", [("time", 2, 70, 3), ("freq", 1, 4, 66), ("time", 1, 1, 5)])
def test_gated_matches_oracle_walk(axis, B, T, Fb):
    """roformer_oracle._attention on each sequence: [b, n, 3, h, dh] -> softmax(q k^T dh^-0.5) v * sigmoid(gate)"""
    rng = np.random.default_rng(T * 7 + Fb)
    heads = 2
    M = B * T * Fb
    qkv = rng.standard_normal((M + 3, 3 * heads * 64))   # 3 padding rows no sequence reads
    gate = 3 * rng.standard_normal((M + 3, heads + 2))
    got = R.rof_attention(qkv, gate, B, T, Fb, axis)
    x = torch.from_numpy(qkv[:M]).reshape(B, T, Fb, 3 * heads * 64)
    g = torch.from_numpy(gate[:M, :heads]).reshape(B, T, Fb, heads)
    if axis == "time":                                   # sequences (b, f) of length T
        xs, gs = x.permute(0, 2, 1, 3).reshape(B * Fb, T, -1), g.permute(0, 2, 1, 3).reshape(B * Fb, T, heads)
    else:                                                # sequences (b, t) of length Fb
        xs, gs = x.reshape(B * T, Fb, -1), g.reshape(B * T, Fb, heads)
    b, n, _ = xs.shape
    q, k, v = xs.reshape(b, n, 3, heads, 64).permute(2, 0, 3, 1, 4)
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * (64 ** -0.5)
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v)
    out = out * gs.permute(0, 2, 1).unsqueeze(-1).sigmoid()
    out = out.permute(0, 2, 1, 3).reshape(b, n, heads * 64)
    if axis == "time":
        out = out.reshape(B, Fb, T, -1).permute(0, 2, 1, 3)
    ref = out.reshape(M, heads * 64).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T,dh,dscale", [(1, 4, 1.0), (67, 8, 1.0), (40, 16, 20.0)])
def test_decay_matches_local_state_formula(T, dh, dscale):
    """hdemucs_oracle._local_state: dots = k.q / sqrt(dh) + einsum(-(f+1)|t - s| / sqrt(4), sigmoid(decay) / 2), diagonal -100,
    softmax over the keys t of every query s"""
    rng = np.random.default_rng(T + dh)
    B, heads = 2, 4
    C = heads * dh
    q, k, v = (rng.standard_normal((B * T, C)) for _ in range(3))
    dec = dscale * rng.standard_normal((B * T, 4 * heads))
    got = R.mha(q, k, v, B, T, T, heads, dh, decay=dec)
    # the oracle's layout: channels-first [B, heads, dh, T], decay logits [B, heads, 4, T]
    def cf(x, c):
        return torch.from_numpy(x).reshape(B, T, heads, c).permute(0, 2, 3, 1)
    qt, kt, vt, dt = cf(q, dh), cf(k, dh), cf(v, dh), cf(dec, 4)
    idx = torch.arange(T, dtype=torch.float64)
    delta = idx[:, None] - idx[None, :]
    dots = torch.einsum("bhct,bhcs->bhts", kt, qt) / dh ** 0.5
    decays = torch.arange(1, 5, dtype=torch.float64)
    dq = torch.sigmoid(dt) / 2
    dk = -decays.view(-1, 1, 1) * delta.abs() / 4 ** 0.5
    dots = dots + torch.einsum("fts,bhfs->bhts", dk, dq)
    dots.masked_fill_(torch.eye(T, dtype=torch.bool), -100)
    w = torch.softmax(dots, dim=2)
    res = torch.einsum("bhts,bhct->bhcs", w, vt)            # [B, heads, dh, T]
    ref = res.permute(0, 3, 1, 2).reshape(B * T, C).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-12)


def test_worst_row_error_sees_one_row():
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((300, 2 * 64))
    got = ref.copy()
    got[299, 64 + 5] += 1e-3 * np.abs(ref[299, 64:]).max()
    assert R.worst_row_error(got, ref, 2) == pytest.approx(1e-3, rel=1e-9)
    assert R.worst_row_error(ref, ref, 2) == 0.0
    got[0, 0] = np.nan
    assert R.worst_row_error(got, ref, 2) == np.inf


def test_mutants():
    """drop_last equals attention over the first nk - 1 keys; tile_local equals exact softmax on one tile and leaves it as soon as
    the maximum moves to a later tile"""
    rng = np.random.default_rng(3)
    B, heads, dh, nq, nk = 1, 2, 48, 20, 130
    q, k, v = (rng.standard_normal((B * n, heads * dh)) for n in (nq, nk, nk))
    np.testing.assert_allclose(R.mha(q, k, v, B, nq, nk, heads, dh, mutant="drop_last"),
                               R.mha(q, k[:-1], v[:-1], B, nq, nk - 1, heads, dh), rtol=1e-13, atol=1e-13)
    short = R.mha(q, k[:64], v[:64], B, nq, 64, heads, dh)
    np.testing.assert_allclose(R.mha(q, k[:64], v[:64], B, nq, 64, heads, dh, mutant="tile_local"), short, rtol=1e-13, atol=1e-13)
    k[-1] = 4 * q.mean(0)                                  # the maximum of every query in the last tile
    ref = R.mha(q, k, v, B, nq, nk, heads, dh)
    assert R.worst_row_error(R.mha(q, k, v, B, nq, nk, heads, dh, mutant="tile_local"), ref, heads) > 1e-2
    assert R.worst_row_error(R.mha(q, k, v, B, nq, nk, heads, dh, mutant="drop_last"), ref, heads) > 1e-2


def test_sigmoid_saturated():
    """the gates of the GPU test reach +-30: the reference sigmoid keeps its relative accuracy there"""
    x = np.array([-80.0, -30.0, -1.0, 0.0, 1.0, 30.0, 80.0])
    np.testing.assert_allclose(R._sigmoid(x), torch.sigmoid(torch.from_numpy(x)).numpy(), rtol=1e-14, atol=0)
