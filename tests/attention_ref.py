"""Float64 numpy references of the attention kernels (asx_op_attention / asx_op_mha), the worst-row error measure of
tests/test_gpu_attention.py, and two deliberately wrong "mutant" attentions that show the bars of that test can catch a
broken kernel.  Checked against torch float64 and the oracles' formulas in tests/test_host_attention_ref.py."""
import numpy as np

KEY_TILE = 64   # keys per tile of every flash-attention kernel (kernels_rof.h, kernels_ht.h)


def _sdpa(q, k, v, scale, bias=None, mutant=None):
    """softmax(q k^T * scale + bias) v over the last two axes, float64.  q [..., Lq, d], k / v [..., Lk, d], bias [..., Lq, Lk].
    mutant "drop_last": the last key is left out; "tile_local": the online-max correction between key tiles is skipped (every
    64-key tile is exponentiated against its own maximum and the tiles' sums are added unscaled)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = np.einsum("...id,...jd->...ij", q, k) * scale
    if bias is not None:
        s = s + bias
    if mutant == "drop_last":
        s = s[..., :-1]
        v = v[..., :-1, :]
    if mutant == "tile_local":
        num = np.zeros(s.shape[:-1] + (v.shape[-1],))
        den = np.zeros(s.shape[:-1] + (1,))
        for j0 in range(0, s.shape[-1], KEY_TILE):
            st = s[..., j0:j0 + KEY_TILE]
            p = np.exp(st - st.max(-1, keepdims=True))
            num += p @ v[..., j0:j0 + KEY_TILE, :]
            den += p.sum(-1, keepdims=True)
        return num / den
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p @ v) / p.sum(-1, keepdims=True)


def _sigmoid(x):
    """1 / (1 + exp(-x)) without cancellation for large |x| (0.5 (1 + tanh(x / 2)) loses ~6e-4 relative at x = -30)"""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def rof_attention(qkv, gate, B, T, Fb, axis, mutant=None):
    """The Roformer attention (bs_roformer.py Attention.forward after the projections): tokens [B, T, Fb] with rows
    (b * T + t) * Fb + f of qkv [M, 3 * heads * 64] and gate [M, >= heads]; sequences along time (axis "time") or frequency.
    Returns [B * T * Fb, heads * 64] float64: softmax(q k^T / 8) v * sigmoid(gate) per (token, head)."""
    n = B * T * Fb
    heads = qkv.shape[1] // 192
    x = np.asarray(qkv[:n], np.float64).reshape(B, T, Fb, 3, heads, 64)
    g = np.asarray(gate[:n, :heads], np.float64).reshape(B, T, Fb, heads)
    if axis == "time":
        x = x.transpose(3, 0, 2, 4, 1, 5)      # [3, B, Fb, heads, T, 64]
        g = g.transpose(0, 2, 3, 1)            # [B, Fb, heads, T]
    else:
        x = x.transpose(3, 0, 1, 4, 2, 5)      # [3, B, T, heads, Fb, 64]
        g = g.transpose(0, 1, 3, 2)            # [B, T, heads, Fb]
    o = _sdpa(x[0], x[1], x[2], 64 ** -0.5, mutant=mutant) * _sigmoid(g)[..., None]
    o = o.transpose(0, 3, 1, 2, 4) if axis == "time" else o.transpose(0, 1, 3, 2, 4)
    return o.reshape(n, heads * 64)


def decay_bias(decay, nq, heads):
    """LocalState score terms (demucs.py:197-221; kernels_ht.h MhaArgs): [B, heads, nq, nq] with -|key - query| * D_query,
    D = 1/4 sum_f (f + 1) sigmoid(logit_f) from the 4 logits of each (query, head).  The diagonal, whose score is replaced by
    -100, is left to mha()."""
    d = _sigmoid(np.asarray(decay, np.float64)[:, :4 * heads]).reshape(-1, nq, heads, 4)
    slope = 0.25 * (d * np.arange(1, 5)).sum(-1)                       # [B, nq, heads]
    idx = np.arange(nq)
    dist = np.abs(idx[None, :] - idx[:, None]).astype(np.float64)     # [query, key]
    return -slope.transpose(0, 2, 1)[..., None] * dist


def mha(q, k, v, B, nq, nk, heads, dh, decay=None, mutant=None):
    """Multi-head attention of the MhaArgs layout: q [B * nq, >= heads * dh], k / v [B * nk, ...]; head h owns columns
    [h * dh, (h + 1) * dh).  Plain: softmax(q k^T / sqrt(dh)) v.  With decay logits [B * nq, >= 4 * heads] (LocalState, nq == nk):
    score = q . k / sqrt(dh) - |key - query| * D_query, the diagonal set to -100.  Returns [B * nq, heads * dh] float64."""
    def heads_of(x, n):
        return np.asarray(x, np.float64)[:, :heads * dh].reshape(B, n, heads, dh).transpose(0, 2, 1, 3)
    qh, kh, vh = heads_of(q, nq), heads_of(k, nk), heads_of(v, nk)
    bias = None
    scale = dh ** -0.5
    if decay is not None:
        s = np.einsum("bhid,bhjd->bhij", qh, kh) * scale + decay_bias(decay, nq, heads)
        s[..., np.arange(nq), np.arange(nq)] = -100.0
        # the scores are final: hand them over as the bias of a zero product
        bias, qh, scale = s, np.zeros_like(qh), 1.0
    o = _sdpa(qh, kh, vh, scale, bias=bias, mutant=mutant)
    return o.transpose(0, 2, 1, 3).reshape(B * nq, heads * dh)


def worst_row_error(got, ref, heads):
    """max over (row, head) of max |got - ref| / max |ref| of that (row, head): one bad tail row is not averaged away.
    A reference row of zeros is measured absolutely."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    rows = ref.shape[0]
    g = got.reshape(rows, heads, -1)
    r = ref.reshape(rows, heads, -1)
    den = np.abs(r).max(-1)
    den = np.where(den > 0, den, 1.0)
    err = np.abs(g - r).max(-1) / den
    return float(np.nanmax(np.where(np.isnan(err), np.inf, err)))
