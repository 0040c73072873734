"""Plain numpy references of the recurrent kernels (asx_op_hd_lstm_layer / asx_op_hd_lstm_frames / asx_op_vr_lstm /
asx_op_vr_lstm_layout): one bidirectional LSTM layer in float64 (or, with dtype=np.float32, the "plain fp32 evaluation" that sets
the bar of tests/test_gpu_lstm_kernels.py), the BLSTM framing of Demucs v3 / HDemucs with the engine's row layout, the two layout
maps of the VR 5.1 LSTMModule, and four deliberately wrong "mutant" recurrences that show the bar can catch a broken kernel.
Checked against torch.nn.LSTM in float64 and torch.Tensor.unfold in tests/test_host_lstm_ref.py."""
import numpy as np

ULP = 2.0 ** -23            # one fp32 ulp at 1; |h| < 1
MARGIN = 8.0                # the kernel may be this many times worse than the plain fp32 evaluation (or than one ulp)
COND_CAP = 1e-5             # inputs on which the plain fp32 evaluation strays further from float64 than this cannot judge a kernel
MUTANTS = ("drop_k_tail", "stale_c", "fwd_only_index", "pad_leak")
FINE_MUTANT = "f16_h"       # a fault a thousand times smaller than those: shows how far the bar could be loosened before it goes blind
MUTANT_CASE = (17, 80, 5)   # (N, H, steps) of the mutant test, at scale (1, 1)
WIDTH, STRIDE = 200, 100    # BLSTM(max_steps=200): frames of 200 with stride 100


def make_inputs(N, H, steps, s=1.0, s_x=1.0, seed=0):
    """whh [2, 4H, H] ~ U(-s / sqrt(H), s / sqrt(H)) and xp [steps * N, 2, 4H] ~ s_x * N(0, 1), float32"""
    rng = np.random.default_rng([seed, N, H, steps])
    whh = rng.uniform(-s / np.sqrt(H), s / np.sqrt(H), (2, 4 * H, H)).astype(np.float32)
    xp = (s_x * rng.standard_normal((steps * N, 2, 4 * H))).astype(np.float32)
    return xp, whh


def _sigmoid(x):
    """1 / (1 + exp(-x)) without overflow, in the dtype of x"""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(x.dtype)


def lstm_layer(xp, whh, N, H, steps, dtype=np.float64, mutant=None):
    """One bidirectional nn.LSTM layer from zero state, every operation in `dtype`.  xp [steps * N, 2, 4H] (input projection plus
    both biases per direction, gate order i, f, g, o), whh [2, 4H, H].  Direction 1 walks steps-1 .. 0.  Returns (out [steps, N, 2H]
    with the forward half | reverse half, final c [2, N, H]).  Mutants: "drop_k_tail" ignores the last 16 columns of W_hh;
    "stale_c" computes h = o * tanh(c_prev); "fwd_only_index" lets direction 1 read xp[s] instead of xp[steps-1-s]; "pad_leak" gives
    sequence N-1 the h of sequence N-2; "f16_h" rounds h to fp16 before the recurrent product (a 16-bit matrix pipe without the
    split into parts)."""
    assert mutant is None or mutant in MUTANTS or mutant == FINE_MUTANT
    xp = np.asarray(xp, dtype).reshape(steps, N, 2, 4 * H)
    whh = np.array(whh, dtype).reshape(2, 4 * H, H)
    if mutant == "drop_k_tail":
        whh[:, :, H - 16:] = 0
    out = np.zeros((steps, N, 2 * H), dtype)
    h = np.zeros((2, N, H), dtype)
    c = np.zeros((2, N, H), dtype)
    for s in range(steps):
        for d in range(2):
            t = steps - 1 - s if d else s
            src = s if mutant == "fwd_only_index" else t
            hp = h[d].astype(np.float16).astype(dtype) if mutant == "f16_h" else h[d]
            g = xp[src, :, d] + hp @ whh[d].T
            i, f, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), _sigmoid(g[:, 3 * H:])
            c_prev = c[d].copy()
            c[d] = f * c_prev + i * np.tanh(g[:, 2 * H:3 * H])
            h[d] = o * np.tanh(c_prev if mutant == "stale_c" else c[d])
            if mutant == "pad_leak" and N > 1:
                h[d, N - 1] = h[d, N - 2]
            out[t, :, d * H:(d + 1) * H] = h[d]
    return out, c


def worst(a, ref):
    """worst-element |a - ref|; NaN (an element never written) counts as infinite"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64))
    return float(np.where(np.isnan(d), np.inf, d).max())


def bar(e32, scale=1.0):
    """the largest worst-element error a kernel may show where the plain fp32 evaluation shows e32"""
    return MARGIN * max(e32, ULP * scale)


# ---- BLSTM framing (demucs.py BLSTM.forward, utils.unfold) ---------------------------------------------------------------------
def framing(T):
    """(steps, nfr): up to 200 frames run as one sequence; more are cut into ceil(T / 100) frames of 200"""
    return (T, 1) if T <= WIDTH else (WIDTH, -(-T // STRIDE))


def blstm_frames(h, T, ntot=None, n_off=0, rows=None):
    """h [B, T, H] -> rows [steps * ntot, H]: row step * ntot + n_off + b * nfr + k holds step `step` of frame k of batch item b
    (zero beyond T); rows of other groups keep what `rows` held (default NaN).  Returns (rows, steps, nfr)."""
    h = np.asarray(h)
    B, T_, H = h.shape
    assert T_ == T
    steps, nfr = framing(T)
    ntot = B * nfr if ntot is None else ntot
    assert n_off + B * nfr <= ntot
    rows = np.full((steps * ntot, H), np.nan, h.dtype) if rows is None else np.array(rows)
    r3 = rows.reshape(steps, ntot, H)
    padded = np.zeros((B, (nfr - 1) * STRIDE + steps, H), h.dtype)
    padded[:, :T] = h
    for b in range(B):
        for k in range(nfr):
            r3[:, n_off + b * nfr + k] = padded[b, k * STRIDE:k * STRIDE + steps]
    return rows, steps, nfr


def blstm_unframe(rows, h, T, ntot=None, n_off=0):
    """h [B, T, H] + the stitched frames of rows [steps * ntot, H] (layout of blstm_frames): frame 0 gives its steps [0, 150), the
    last frame [50, 200), the others [50, 150); the concatenation is cropped to T.  One add in the dtype of the inputs."""
    h = np.asarray(h)
    B, T_, H = h.shape
    assert T_ == T
    steps, nfr = framing(T)
    ntot = B * nfr if ntot is None else ntot
    r3 = np.asarray(rows).reshape(steps, ntot, H)
    out = np.empty_like(h)
    lim = STRIDE // 2
    for b in range(B):
        fr = [r3[:, n_off + b * nfr + k] for k in range(nfr)]
        if nfr > 1:
            fr = [f[:-lim] if k == 0 else f[lim:] if k == nfr - 1 else f[lim:-lim] for k, f in enumerate(fr)]
        out[b] = h[b] + np.concatenate(fr, 0)[:T]
    return out


# ---- VR 5.1 LSTMModule layouts (layers_new.py LSTMModule.forward) ---------------------------------------------------------------
def vr_lstm_in(hc, ch0=0):
    """channel ch0 of hc [B, H, W, ld] -> [W, B, H] (nframes, batch, nbins)"""
    return np.ascontiguousarray(np.asarray(hc)[..., ch0].transpose(2, 0, 1))


def vr_lstm_out(ys, dst, ch0):
    """ys [W, B, H] -> channel ch0 of a copy of dst [B, H, W, ld]; channels ch0+1 .. ch0+3 zeroed, the others untouched"""
    dst = np.array(dst)
    dst[..., ch0] = np.asarray(ys).transpose(1, 2, 0)
    dst[..., ch0 + 1:ch0 + 4] = 0
    return dst
