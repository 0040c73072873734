"""The cases of tests/test_gpu_stft_kernels.py: geometry, descriptor, inputs and float64 reference of every STFT / iSTFT launch tested
(tests/stft_ref.py holds the formulas and the measures).  Pure numpy / torch on the CPU: tests/test_host_stft_ref.py walks the same
tables without a GPU.

A case is a dict: `dir` "fwd" / "inv" / "ht_spec" / "ht_ispec", the engine geometry (n_fft, hop, dim_f, win_length, window, env = the
environment the engine is created under), the descriptor fields of asx_stft_desc, and `expect` = (kernel name, seam launches).  A case
with `generic` set runs once more on an engine created with ASX_FFT3=0 and must meet the same bar there."""
import functools

import numpy as np

from tests import stft_ref as R

FFT3_G = 16            # frames per workgroup of the fast inverse (knobs.h fft3_g): groups = max(1, T // 16)


def _case(name, dir, n_fft, hop, dim_f, T, expect, **kw):
    c = dict(name=name, dir=dir, n_fft=n_fft, hop=hop, dim_f=dim_f, T=T, expect=expect, B=kw.pop("B", None), C=kw.pop("C", hop * (T - 1)),
             win_length=0, window=None, env={}, layout=0, subbands=0, gap=0, zero_low=0, sign=1.0, n_inst=0, combine=0, normalized=0,
             mode="chunks", front=0, starts=None, song_len=None, song_of=None, n_act=None, generic=False, rot=0, seed=len(name) * 7919 + T)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return c


def segment_size(c):
    """the engine's segment_size: the case's T where the engine accepts it (chunk longer than n_fft), else the smallest it accepts"""
    return max(c["T"], c["n_fft"] // c["hop"] + 2)


# ---- forward cases -----------------------------------------------------------------------------------------------------------------
PLANS = [(16, "8"), (20, "2.5"), (24, "4.3"), (64, "16.2"), (96, "16.3"), (160, "16.5"), (256, "16.8"), (600, "4.3.5.5"),
         (2048, "16.16.4"), (4096, "16.16.8"), (7680, "16.16.3.5"), (8192, "16.16.16")]

FWD, INV = [], []
for n, stages in PLANS:
    FWD.append(_case(f"fwd-plan-{n}-{stages}", "fwd", n, n // 4, n // 2 + 1, 6, ("stft", 0)))
    INV.append(_case(f"inv-plan-{n}-{stages}", "inv", n, n // 4, n // 2 + 1, 6, ("istft+ola", 0)))
FWD.append(_case("fwd-6144-generic-kernels", "fwd", 6144, 1024, 3073, 6, ("stft", 0), env={"ASX_FFT3": "0"}))
INV.append(_case("inv-6144-generic-kernels", "inv", 6144, 1024, 3073, 6, ("istft+ola", 0), env={"ASX_FFT3": "0"}))
# other geometries of the generic family
FWD += [
    _case("fwd-dimf-half", "fwd", 96, 24, 48, 6, ("stft", 0)),
    _case("fwd-dimf-low-zero3-neg", "fwd", 96, 24, 20, 6, ("stft", 0), zero_low=3, sign=-1.0),
    _case("fwd-l1-mdx-zero3", "fwd", 160, 40, 80, 6, ("stft", 0), layout=1, zero_low=3),
    _case("fwd-l1-sub1-gap", "fwd", 160, 40, 80, 6, ("stft", 0), layout=1, subbands=1, gap=24),
    _case("fwd-l1-sub2", "fwd", 160, 40, 80, 6, ("stft", 0), layout=1, subbands=2),
    _case("fwd-l1-sub4-gap", "fwd", 160, 40, 80, 6, ("stft", 0), layout=1, subbands=4, gap=8),
    _case("fwd-l2-441", "fwd", 2048, 441, 1025, 8, ("stft", 0), layout=2),
    _case("fwd-l2-441-normalized", "fwd", 2048, 441, 1025, 8, ("stft", 0), layout=2, normalized=1),
    _case("fwd-winlen48", "fwd", 64, 16, 33, 6, ("stft", 0), win_length=48),
    _case("fwd-hamming", "fwd", 64, 16, 33, 6, ("stft", 0), window="hamming"),
    # song mode: unaligned starts, a song shorter than one chunk, a last chunk past the song's end; a two-song pool, chunks interleaved
    _case("fwd-song-unaligned", "fwd", 96, 24, 49, 6, ("stft", 0), mode="song", front=48, starts=[0, 37, 101, 333], song_len=[401], B=4),
    _case("fwd-song-short", "fwd", 96, 24, 49, 6, ("stft", 0), mode="song", front=48, starts=[0, 5], song_len=[71], B=2),
    _case("fwd-pool-two-songs", "fwd", 96, 24, 49, 6, ("stft_pool", 0), mode="pool", front=48, starts=[0, 0, 96, 111, 192, 200],
          song_of=[0, 1, 0, 1, 0, 1], song_len=[300, 257], B=6, layout=1, subbands=1),
    _case("fwd-l2-song-front0", "fwd", 2048, 441, 1025, 8, ("stft", 0), layout=2, mode="song", front=0, starts=[0, 1500, 3001],
          song_len=[5000], B=3),
]
INV += [
    _case("inv-dimf-half", "inv", 96, 24, 48, 6, ("istft+ola", 0)),
    _case("inv-dimf-low-combine", "inv", 96, 24, 20, 6, ("istft+ola", 0), combine=1),
    _case("inv-l1-mdx-nact", "inv", 160, 40, 80, 6, ("istft+ola", 0), layout=1, B=3, n_act=[150, 200, -1]),
    _case("inv-l1-sub1-gap-inst2", "inv", 160, 40, 80, 6, ("istft+ola", 0), layout=1, subbands=1, gap=24, n_inst=2, B=2),
    _case("inv-l1-sub2-inst2", "inv", 160, 40, 80, 6, ("istft+ola", 0), layout=1, subbands=2, n_inst=2, B=2),
    _case("inv-l1-sub4-gap", "inv", 160, 40, 80, 6, ("istft+ola", 0), layout=1, subbands=4, gap=8),
    _case("inv-l2-441-mask", "inv", 2048, 441, 1025, 8, ("istft+ola", 0), layout=2, n_inst=2, B=2),
    _case("inv-l2-441-mask-normalized", "inv", 2048, 441, 1025, 8, ("istft+ola", 0), layout=2, n_inst=2, normalized=1, B=2),
    _case("inv-441-short-c", "inv", 2048, 441, 1025, 8, ("istft+ola", 0), C=3000, B=2),
    _case("inv-winlen48", "inv", 64, 16, 33, 6, ("istft+ola", 0), win_length=48),
    _case("inv-hamming", "inv", 64, 16, 33, 6, ("istft+ola", 0), window="hamming"),
]
# the 6144 / 1024 fast path: stft3p (ASX_FFT3P on, frame groups over an LDS ring: 1 group at T 6 and 16, 2 at T 33, so song and pool
# positions are also mapped by a group that starts inside the chunk) and stft3 (ASX_FFT3P=0), each with its pool twin, at T 6 / 16 / 33 and
# dim_f 3072 / 2048, from explicit chunks, from windows of one song (unaligned and 16-byte aligned starts, the last chunk half past the
# song's end) and from a two-song pool with interleaved chunks (one song of odd length, one chunk starting at its song's last samples)
for T in (6, 16, 33):
    Cf = 1024 * (T - 1)
    for F in (3072, 2048):
        for kern, env in (("stft3p", {}), ("stft3", {"ASX_FFT3P": "0"})):
            tag = f"fwd{kern[4:]}"
            FWD.append(_case(f"{tag}-T{T}-F{F}", "fwd", 6144, 1024, F, T, (kern, 0), layout=1, zero_low=3, generic=True, env=env,
                             B=9 if T < 33 else 4, rot=0 if T < 33 else (4 + F // 1024 if kern == "stft3p" else 9 + F // 1024)))
            FWD.append(_case(f"{tag}-song-T{T}-F{F}", "fwd", 6144, 1024, F, T, (kern, 0), layout=1, zero_low=3, generic=True, env=env,
                             mode="song", front=3072, song_len=[2 * Cf + 1027], B=4,
                             starts=[0, Cf // 2 + 3, Cf + 1024, 3072 + 2 * Cf + 1027 - Cf // 2]))
            FWD.append(_case(f"{tag}-pool-T{T}-F{F}", "fwd", 6144, 1024, F, T, (kern + "_pool", 0), layout=1, zero_low=3, generic=True,
                             env=env, mode="pool", front=3072, song_len=[Cf + 2049, Cf + 1024], song_of=[0, 1, 0, 1], B=4,
                             starts=[0, 0, Cf + 2049, 1024]))
for T, seams in ((6, 0), (31, 0), (32, 1), (33, 1), (70, 1)):
    INV.append(_case(f"inv3p-T{T}", "inv", 6144, 1024, 3072 if T != 70 else 2048, T, ("istft3p", seams), layout=1, generic=True))
INV += [
    _case("inv3p-T33-chunk-window", "inv", 6144, 1024, 3072, 33, ("istft3p", 1), layout=1, generic=True, B=3,
          n_act=[32 * 1024, 20000, -1]),
    _case("inv3-combine", "inv", 6144, 1024, 3072, 33, ("istft3", 1), layout=1, combine=1, generic=True, B=3, n_act=[32 * 1024, 777, -1]),
    _case("inv3-dimf3070", "inv", 6144, 1024, 3070, 33, ("istft3", 1), layout=1, generic=True),
    _case("inv3-no-prefetch", "inv", 6144, 1024, 3072, 33, ("istft3", 1), layout=1, env={"ASX_FFT3P": "0"}, generic=True),
    _case("inv-6144-short-c-falls-back", "inv", 6144, 1024, 3072, 16, ("istft+ola", 0), layout=1, C=15 * 1024 - 8, B=2),
]

# ---- Demucs ------------------------------------------------------------------------------------------------------------------------
HT = [dict(name="ht-spec-4096", dir="ht_spec", nfft=4096, L=7 * 1024 + 333, B=2, seed=11)]
HT += [dict(name=f"ht-spec-1024-L{L}", dir="ht_spec", nfft=1024, L=L, B=2, seed=13 + L) for L in (2000, 877, 100, 3)]
HT += [dict(name=f"ht-ispec-4096-S{S}-{tag}", dir="ht_ispec", nfft=4096, L=7 * 1024 + 333, B=2, S=S, mean=m, std=sd, time=tb, seed=17 + S)
       for S, tag, m, sd, tb in ((2, "m0.3", 0.3, 2.5, True), (4, "m30", 30.0, 1.0, True), (2, "no-time", 0.3, 2.5, False))]
HT += [dict(name=f"ht-ispec-1024-L{L}", dir="ht_ispec", nfft=1024, L=L, B=2, S=2, mean=0.3, std=2.5, time=True, seed=19 + L)
       for L in (2000, 100)]

ALL = FWD + INV + HT
BY_NAME = {c["name"]: c for c in ALL}
assert len(BY_NAME) == len(ALL)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def window_of(c):
    return R.hamming_table(c["n_fft"]) if c["window"] == "hamming" else R.hann_table(c["n_fft"], c["win_length"])


def _signals(c, C, rng):
    """the forward inputs, one per (batch item, channel) slot in turn: white noise, bin-centred tones, unit impulses, 1 + 1e-3 noise,
    noise under exp(-30 t / n)"""
    n, F, zl = c["n_fft"], c["dim_f"], c["zero_low"]
    t = np.arange(C, dtype=np.float64)
    sig = [rng.standard_normal(C)]
    for k in (0, 1, max(zl - 1, 0), zl, F - 1, n // 2 - 1, n // 2):
        sig.append(np.cos(2.0 * np.pi * k * t / n))                      # bin n / 2: alternating sign
    for p in (0, 1, n // 2 - 1, n // 2, C - n // 2, C - 2, C - 1):
        x = np.zeros(C)
        x[p] = 1.0
        sig.append(x)
    sig.append(1.0 + 1e-3 * rng.standard_normal(C))
    sig.append(rng.standard_normal(C) * np.exp(-t * 30.0 / n))
    return sig


def _default_B(c):
    if c["B"]:
        return c["B"]
    return 9 if c["dir"] == "fwd" else max(1, (len(_inv_kinds(c)) + 1) // 2)


def _inv_kinds(c):
    """the inverse inputs per (item, stem, channel) slot in turn: a noise spectrum, then spectra that are zero except one frame -- t in
    {0, 1, T - 1} and either side of every seam between the fast path's frame groups"""
    T = c["T"]
    ng = max(1, T // FFT3_G) if (c["n_fft"], c["hop"]) == (6144, 1024) else 1
    ts = {0, 1, T - 1}
    for g in range(1, ng):
        ts |= {g * T // ng - 1, g * T // ng}
    return ["noise"] + sorted(ts)


@functools.lru_cache(maxsize=1)
def build(name):
    """(inputs, reference) of a case, kept while its test runs: a dict with whatever the runner needs (see test_gpu_stft_kernels.py)"""
    c = BY_NAME[name]
    rng = np.random.default_rng(c["seed"])
    if c["dir"] == "fwd":
        return _build_fwd(c, rng)
    if c["dir"] == "inv":
        return _build_inv(c, rng)
    return _build_ht(c, rng)


def _build_fwd(c, rng):
    n, hop, F, T, C, B = c["n_fft"], c["hop"], c["dim_f"], c["T"], c["C"], _default_B(c)
    w = window_of(c)
    if c["mode"] == "chunks":
        sig = _signals(c, C, rng)
        wave = np.stack([sig[(i + c["rot"]) % len(sig)] for i in range(B * 2)]).reshape(B, 2, C).astype(np.float32)
        frames = R.frames_chunks(wave, n, hop, T)
        flat = wave.reshape(-1)
    else:
        songs = []
        for N in c["song_len"]:
            s = rng.standard_normal((2, N))
            s[0, 0] += 40.0                                              # impulses on the song's first and last samples
            s[1, N - 1] -= 40.0
            songs.append(s.astype(np.float32))
        frames = R.frames_song(songs, c["song_of"] or [0] * B, c["starts"], c["front"], C, n, hop, T)
        flat = np.concatenate([s.reshape(-1) for s in songs])
    scale = c["sign"] * (n ** -0.5 if c["normalized"] else 1.0)
    X, P, e32 = R.forward64(frames, w, scale)
    item = 4 * T * F
    bstride = item + c["gap"] if c["gap"] else 0
    idx = R.spec_index(c["layout"], B, 1, T, F, c["subbands"], bstride)[:, 0]
    size = (B - 1) * (bstride or item) + item
    desc = dict(b=B, t=T, c=C, layout=c["layout"], subbands=c["subbands"], zero_low=c["zero_low"], sign=c["sign"], bstride=bstride,
                stft_normalized=c["normalized"], mode=c["mode"], front=c["front"], starts=c["starts"], song_len=c["song_len"],
                song_of=c["song_of"], n_songs=len(c["song_len"] or []))
    return dict(wave=flat, desc=desc, idx=idx, size=size, X=X, P=P, e32=e32)


def _build_inv(c, rng):
    n, hop, F, T, C, B = c["n_fft"], c["hop"], c["dim_f"], c["T"], c["C"], _default_B(c)
    S = max(c["n_inst"], 1)
    items = B * (2 if c["combine"] else 1)
    w = window_of(c)
    kinds = _inv_kinds(c)
    lay2 = c["layout"] == 2
    Ssp = 1 if lay2 else S                                               # layout 2: the S stems share the item's spectrum
    Xin = np.zeros((items, Ssp, 2, T, F), np.complex64)
    slot = 0
    for i in range(items):
        for s in range(Ssp):
            for ch in range(2):
                k = kinds[slot % len(kinds)] if not lay2 else "noise"
                z = (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))).astype(np.complex64) * (1.0 + slot)
                if k != "noise":
                    z[np.arange(T) != k] = 0
                Xin[i, s, ch] = z                                        # DC and Nyquist keep their imaginary parts
                slot += 1
    item = Ssp * 4 * T * F
    bstride = item + c["gap"] if c["gap"] else 0
    idx = R.spec_index(c["layout"], items, Ssp, T, F, c["subbands"], bstride)
    size = (items - 1) * (bstride or item) + item
    spec = np.full(size, np.nan, np.float32)                             # the gaps between items are never read
    spec[idx[..., 0]] = Xin.real
    spec[idx[..., 1]] = Xin.imag
    X = Xin.astype(np.complex128)
    mask = None
    if lay2:
        M = (rng.standard_normal((B, S, 2, T, F)) + 1j * rng.standard_normal((B, S, 2, T, F))).astype(np.complex64)
        mask = np.zeros(B * S * T * F * 4, np.float32)
        mi = R.mask_index(B, S, T, F)
        mask[mi[..., 0]] = M.real
        mask[mi[..., 1]] = M.imag
        X = X * M.astype(np.complex128)                                  # [B, 1, ...] x [B, S, ...]
    if c["combine"]:
        X = 0.5 * X[:B] - 0.5 * X[B:]
    Z = R.c2r_spectrum(X.reshape(B * S * 2, T, F), n)
    n_act = None
    if c["n_act"] is not None:
        n_act = np.repeat(np.asarray(c["n_act"], np.int64), 2)           # per (chunk, channel) row
    out, s, e32 = R.inverse64(Z, w, hop, C, scale=(n ** 0.5 if c["normalized"] else 1.0), n_act=n_act)
    desc = dict(b=B, t=T, c=C, layout=c["layout"], subbands=c["subbands"], n_inst=c["n_inst"], combine=c["combine"], bstride=bstride,
                stft_normalized=c["normalized"], n_act=c["n_act"])
    env = R.envelope(w, hop, T)[n // 2:n // 2 + C]
    return dict(spec=spec, mask=mask, desc=desc, out=out.reshape(B * S, 2, C), s=s.reshape(B * S, 2, C), e32=e32, env=env)


def _build_ht(c, rng):
    nfft, L, B = c["nfft"], c["L"], c["B"]
    hop = nfft // 4
    T = -(-L // hop)
    if c["dir"] == "ht_spec":
        sig = _signals(dict(n_fft=nfft, dim_f=nfft // 2, zero_low=0), L, rng) if L > nfft // 2 else [rng.standard_normal(L) for _ in range(4)]
        seg = np.stack([sig[(i * 5) % len(sig)] for i in range(B * 2)]).reshape(B, 2, L).astype(np.float32)
        el, lv = R.demucs_extension(L, nfft)
        X, P, e32 = R.forward64(R.frames_demucs(seg, nfft, el, lv), R.hann_table(nfft), nfft ** -0.5)
        return dict(seg=seg, el=el, lv=lv, X=X, P=P, e32=e32, T=T)
    S = c["S"]
    x = rng.standard_normal((B, T, nfft // 2, 4 * S)).astype(np.float32)
    x[0, :, :, 0:2] = 0
    x[0, T // 2, :, 0:2] = rng.standard_normal((nfft // 2, 2))           # stem 0, left of item 0: one frame alone
    xt = (rng.standard_normal((B, L, 2 * S)) if c["time"] else np.zeros((B, L, 2 * S))).astype(np.float32)
    n_stat = float(T * (nfft // 2) * 4)
    m = np.array([c["mean"], -c["mean"]][:B])
    sd = np.array([c["std"], 0.5 * c["std"]][:B])
    acc_f = np.stack([m * n_stat, (n_stat - 1.0) * sd * sd + n_stat * m * m], axis=1)       # the (sum, sum of squares) of that mean / std
    mt, st = (np.array([0.05, -0.1][:B]), np.array([0.7, 1.3][:B])) if c["time"] else (np.zeros(B), np.zeros(B))
    acc_t = np.stack([mt * 2 * L, (2.0 * L - 1.0) * st * st + 2.0 * L * mt * mt], axis=1)
    out, s, e32 = R.demucs_inverse64(x, nfft, acc_f, n_stat, xt, acc_t, L)
    return dict(x=x, xt=xt, acc_f=acc_f, acc_t=acc_t, n_stat=n_stat, out=out, s=s, e32=e32)
