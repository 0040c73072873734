"""Counts, on the CPU, how often conv3h_kernel's block exponent moves per tile under three rules, on the activations the oracle net
(oracle/mdx_oracle.py, seeded synthetic weights) feeds its 48- / 96- / 144-channel 3x3 convs for one chunk of the seeded synthetic song at
the HQ_3 geometry (n_fft 6144, hop 1024, dim_f 3072, 256 frames): today's running exponent with hysteresis (restart per segment of
64 / 16 / 4 tile rows at levels 0 / 1 / 2, follow a block more than 8 bits quieter), rule (a) = the need rounded down to a multiple of 8
(a block of zeros keeps the exponent before it), rule (b) = the hysteresis restarted every four blocks.  A block is four rows x 40 columns
(a 32-wide strip and its halo quads) x 48 channels.  profiles/NOTES.md round 20 records the output.
    python tools/conv3h_exponent_moves.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from oracle import mdx_oracle as O

d = O.NetDims()
sd = {k: torch.as_tensor(v) for k, v in O.make_convtdf_state(d, seed=0).items()}
n_fft, hop, dim_f, T = 6144, 1024, 3072, 256
C = hop * (T - 1)
mix = O.synth_mix(C + 44100, seed=0)
spec = O.stft_forward(mix[:, 22050:22050 + C][None], n_fft, hop, dim_f)

caps = []
conv2d = F.conv2d


def hook(x, w, b=None, stride=1, padding=0, *a, **k):
    if w.shape[-1] == 3 and w.shape[0] == w.shape[1] and w.shape[0] % 48 == 0 and w.shape[0] <= 144:
        caps.append(x[0].numpy().copy())
    return conv2d(x, w, b, stride, padding, *a, **k)


O.F.conv2d = hook
O.convtdf_forward(np.asarray(spec, np.float32)[:1], sd, d)


def needs(x48):
    """need [block -1 .. tilesT - 1, strip] and whether the block is all zero"""
    c, T, Fq = x48.shape
    tT, tF = (T + 3) // 4, Fq // 32
    xp = np.zeros((c, 4 * (tT + 1) + 4, Fq + 8), np.float32)
    xp[:, 3:3 + T, 4:4 + Fq] = np.abs(x48)
    blk = xp.max(axis=0)[:4 * (tT + 1)].reshape(tT + 1, 4, -1).max(axis=1)
    out, zero = np.zeros((tT + 1, tF), np.int64), np.zeros((tT + 1, tF), bool)
    for s in range(tF):
        m = blk[:, s * 32: s * 32 + 40].max(axis=1)
        zero[:, s] = m == 0
        out[:, s] = np.minimum(np.where(m > 0, 15 - np.frexp(np.where(m > 0, m, 1.0))[1], 15) - 1, 100)
    return out, zero


def hysteresis(need, restart):
    """moves of the running exponent down one walk; restart(k): the block at index k takes its own need whatever came before"""
    mv = 0
    for s in range(need.shape[1]):
        ep = None
        for k in range(need.shape[0]):
            nd = need[k, s]
            if ep is None or restart(k) or nd < ep:
                e = nd
            elif nd > ep + 8:
                e = min(nd, ep + 40)
            else:
                e = ep
            mv += ep is not None and e != ep
            ep = e
    return mv


def rule_a(need, zero, Q=8):
    mv = 0
    for s in range(need.shape[1]):
        ep = None
        for k in range(need.shape[0]):
            e = ep if zero[k, s] and ep is not None else (need[k, s] // Q) * Q
            mv += ep is not None and e != ep
            ep = e
    return mv


res = {}
for x in caps:
    lvl = x.shape[0] // 48 - 1
    tps = {0: 64, 1: 16, 2: 4}[lvl]
    for sl in range(x.shape[0] // 48):
        nd, z = needs(x[sl * 48:(sl + 1) * 48])
        r = res.setdefault(lvl, {"tiles": 0, "today": 0, "a": 0, "b": 0})
        r["tiles"] += (nd.shape[0] - 1) * nd.shape[1]
        # today: a segment of tps tile rows is blocks t0 - 1 .. t0 + tps - 1, a walk of its own
        r["today"] += sum(hysteresis(nd[t0:t0 + tps + 1], lambda k: False) for t0 in range(0, nd.shape[0] - 1, tps))
        r["a"] += rule_a(nd, z)
        r["b"] += hysteresis(nd, lambda k: k % 4 == 0)   # index k is block k - 1: (block + 1) % 4 == 0
for lvl in sorted(res):
    r = res[lvl]
    print(f"level {lvl}: {r['tiles']} tiles; moves per tile: today {r['today'] / r['tiles']:.4f}, (a) {r['a'] / r['tiles']:.4f}, (b) {r['b'] / r['tiles']:.4f}")
