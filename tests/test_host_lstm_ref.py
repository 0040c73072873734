"""tests/lstm_ref.py pinned to things it did not come from: torch.nn.LSTM in float64 for the recurrence, torch.Tensor.unfold and
the stitching of BLSTM.forward for the framing; and the check that keeps test_gpu_lstm_kernels.py::test_bar_catches_mutants
meaningful -- on its input every mutant is far from the reference while the plain fp32 evaluation is close."""
import numpy as np
import pytest
import torch

from tests import lstm_ref as R


@pytest.mark.parametrize("N,H,steps", [(3, 16, 9), (2, 48, 5)])
def test_lstm_layer_matches_torch_float64(N, H, steps):
    torch.manual_seed(N * 1000 + H)
    m = torch.nn.LSTM(H, H, bidirectional=True).double()
    x = torch.randn(steps, N, H, dtype=torch.float64)
    with torch.no_grad():
        y, (_, cn) = m(x)
        xp = torch.stack([x @ getattr(m, "weight_ih_l0" + sfx).T + getattr(m, "bias_ih_l0" + sfx) + getattr(m, "bias_hh_l0" + sfx)
                          for sfx in ("", "_reverse")], 2)                     # [steps, N, 2, 4H]
        whh = torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse])
    out, c = R.lstm_layer(xp.numpy().reshape(steps * N, 2, 4 * H), whh.numpy(), N, H, steps)
    assert out.shape == (steps, N, 2 * H) and c.shape == (2, N, H)
    assert np.abs(out - y.numpy()).max() < 1e-12
    assert np.abs(c - cn.numpy()).max() < 1e-12


def _torch_blstm_identity(h):
    """BLSTM.forward with the LSTM and the linear replaced by the identity and skip=True, on h [B, T, C] (torch float32)"""
    x = h.permute(0, 2, 1)                                                     # B, C, T
    B, C, T = x.shape
    y = x
    if T > 200:
        nframes = -(-T // 100)
        xpad = torch.nn.functional.pad(x, (0, (nframes - 1) * 100 + 200 - T))
        frames = xpad.unfold(-1, 200, 100)                                     # B, C, nframes, 200
        assert frames.shape[2] == nframes
        out = []
        for k in range(nframes):
            f = frames[:, :, k]
            out.append(f[..., :-50] if k == 0 else f[..., 50:] if k == nframes - 1 else f[..., 50:-50])
        x = torch.cat(out, -1)[..., :T]
    return (x + y).permute(0, 2, 1)


@pytest.mark.parametrize("T", [1, 200, 201, 250, 299, 300, 301])
def test_framing_matches_unfold(T):
    B, H = 2, 3
    rng = np.random.default_rng(T)
    h = rng.standard_normal((B, T, H)).astype(np.float32)
    rows, steps, nfr = R.blstm_frames(h, T)
    assert (steps, nfr) == ((T, 1) if T <= 200 else (200, -(-T // 100)))
    assert rows.shape == (steps * B * nfr, H) and not np.isnan(rows).any()
    # the rows are the zero-padded unfold, sequence-major
    if T > 200:
        xpad = torch.nn.functional.pad(torch.from_numpy(h).permute(0, 2, 1), (0, (nfr - 1) * 100 + 200 - T))
        fr = xpad.unfold(-1, 200, 100).permute(3, 0, 2, 1).reshape(200 * B * nfr, H)   # step, b, k, c
        assert np.array_equal(rows, fr.numpy())
    else:
        assert np.array_equal(rows.reshape(T, B, H), h.transpose(1, 0, 2))
    got = R.blstm_unframe(rows, h, T)
    assert np.array_equal(got, _torch_blstm_identity(torch.from_numpy(h)).numpy())
    assert np.array_equal(got, h + h)                                          # every step comes back from exactly one frame
    # the shared-launch layout: the same rows at n_off of a wider matrix, the other groups' rows untouched
    ntot, n_off = B * nfr + 5, 3
    wide, _, _ = R.blstm_frames(h, T, ntot, n_off)
    w3 = wide.reshape(steps, ntot, H)
    assert np.array_equal(w3[:, n_off:n_off + B * nfr].reshape(-1, H), rows)
    assert np.isnan(w3[:, :n_off]).all() and np.isnan(w3[:, n_off + B * nfr:]).all()
    assert np.array_equal(R.blstm_unframe(np.nan_to_num(wide, nan=7.0), h, T, ntot, n_off), got)


def test_vr_layout_maps():
    B, H, W, ld = 2, 3, 5, 12
    rng = np.random.default_rng(0)
    hc = rng.standard_normal((B, H, W, ld)).astype(np.float32)
    xs = R.vr_lstm_in(hc, 4)
    assert xs.shape == (W, B, H)
    assert all(xs[t, b, h] == hc[b, h, t, 4] for t in range(W) for b in range(B) for h in range(H))
    back = R.vr_lstm_out(xs, hc, 4)
    assert np.array_equal(back[..., 4], hc[..., 4]) and (back[..., 5:8] == 0).all()
    assert np.array_equal(back[..., :4], hc[..., :4]) and np.array_equal(back[..., 8:], hc[..., 8:])


def test_mutants_are_far_and_fp32_is_close():
    cases = [(R.MUTANT_CASE, R.MUTANTS), ((16, 48, 7), ("drop_k_tail",))]
    for (N, H, steps), mutants in cases:
        xp, whh = R.make_inputs(N, H, steps)
        ref, cref = R.lstm_layer(xp, whh, N, H, steps)
        o32, c32 = R.lstm_layer(xp, whh, N, H, steps, np.float32)
        assert o32.dtype == np.float32 and c32.dtype == np.float32
        assert R.worst(o32, ref) < R.COND_CAP and R.worst(c32, cref) < R.COND_CAP
        for m in mutants:
            out, _ = R.lstm_layer(xp, whh, N, H, steps, mutant=m)
            assert R.worst(out, ref) > 1e-3, (m, R.worst(out, ref))
        # the fine mutant (h rounded to fp16: relative 2^-11 per operand) sits between the bar and 1000 x the bar, so the GPU mutant
        # test goes red if the bar is loosened by that much
        fine = R.worst(R.lstm_layer(xp, whh, N, H, steps, mutant=R.FINE_MUTANT)[0], ref)
        assert 10 * R.bar(R.worst(o32, ref)) < fine < 1000 * R.bar(R.worst(o32, ref)), fine


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_change_what_they_say(mutant):
    """each mutant leaves alone what it does not touch: the check that it models one fault, not noise"""
    N, H, steps = R.MUTANT_CASE
    xp, whh = R.make_inputs(N, H, steps)
    ref, _ = R.lstm_layer(xp, whh, N, H, steps)
    out, _ = R.lstm_layer(xp, whh, N, H, steps, mutant=mutant)
    if mutant == "pad_leak":
        assert np.array_equal(out[:, :N - 1], ref[:, :N - 1]) and not np.array_equal(out[:, N - 1], ref[:, N - 1])
    elif mutant == "fwd_only_index":
        assert np.array_equal(out[..., :H], ref[..., :H]) and not np.array_equal(out[..., H:], ref[..., H:])
    else:   # the first step from zero state has no recurrent term and no previous cell
        same_first = np.array_equal(out[0, :, :H], ref[0, :, :H])
        assert same_first == (mutant == "drop_k_tail") and not np.array_equal(out[1], ref[1])
