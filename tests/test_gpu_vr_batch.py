"""asx_vr_separate_batch_dev: a pool of songs whose patches share the net passes, on the small fixture of test_gpu_vr.py
(window 64, offset 16, so 32 frames per patch; polyphase converter).

The pooled tests rest on "the stems do not depend on how many patches a pass holds" (engine_vr.h), which
test_patches_per_pass_do_not_change_the_stems pins to equality first; from there the pool is held to np.array_equal against
asx_vr_separate_dev per song on the same engine, and to TOL of test_gpu_vr.py against the reference's golden vectors."""
import filecmp
import os

import numpy as np
import pytest

from oracle import vr_oracle as V
from tests import separate_cases as SC
from tests.test_gpu_vr import SMALL_CAP, TOL, demixer, rel_rms

pytestmark = pytest.mark.gpu
ROI = 32
# frames per song: the minimum; one short of a patch; exactly one patch (T % roi == 0: the extra patch is all padding);
# several patches and a bit; and the second song again at another position
FRAMES = (2, ROI - 1, ROI, 5 * ROI + 7, ROI - 1)


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "vr_small.npz"))


def even_batches(nk, max_b):
    nbatch = -(-nk // max_b)
    return -(-nk // nbatch)


def length_for(eng, frames):
    """a sample count (not a multiple of the hop) that gives `frames` frames"""
    hop = 64
    for n in range(hop * (frames - 1) + 7, hop * frames):
        if eng.vr_plan(n)[0] == frames:
            return n
    raise AssertionError(frames)


def pool_waves(eng, wave, frames=FRAMES):
    """one wave per entry of `frames`, cut from `wave` at different places; equal frame counts get the same wave"""
    out, cut = [], {}
    for i, t in enumerate(frames):
        if t not in cut:
            n = length_for(eng, t)
            start = 1000 * i
            cut[t] = np.ascontiguousarray(wave[:, start:start + n])
            assert cut[t].shape[1] == n and eng.vr_plan(n)[0] == t
        out.append(cut[t])
    return out


def to_dev(waves):
    import torch
    return [torch.from_numpy(w).cuda() for w in waves]


def demixer51_at(A, max_batch, **arch_cfg):
    """demixer51 of test_gpu_vr.py with the patches per pass set"""
    cfg = {"window_size": 64, "batch_size": 2, "aggression": 5, "asx_res_type": "polyphase"}
    cfg.update(arch_cfg)
    return A.VRDemixer({"model_params": V.small_params_v51().param, "primary_stem_name": "Instrumental", "torch_device": 0,
                        "model_data": {"nout": 16, "nout_lstm": 16}}, cfg, state_dict=V.make_vr51_state(192, 16, 16, 9),
                       nn_arch_size=56817, offset=16, max_batch=max_batch)


def singles(dm, waves_d):
    return [dm.separate_stems_dev(w).cpu().numpy() for w in waves_d]


def test_patches_per_pass_do_not_change_the_stems(A, g):
    """The premise: one song through the single-song call at 1, 3 and 48 patches per pass gives the same stems, bit for bit
    (every kernel of the cascade computes a patch's values from that patch alone, in an order that does not depend on the
    batch)."""
    wave = g["wave"][:, :length_for(demixer(A).engine, 5 * ROI + 7)]
    for make in (lambda mb: demixer(A, max_batch=mb, enable_tta=True), lambda mb: demixer51_at(A, mb)):
        got = [np.stack(make(mb).separate_stems(wave)) for mb in (1, 3, 48)]
        assert np.isfinite(got[0]).all() and got[0].any()
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


MID_SIDE = dict(V.small_params().param, mid_side=True, aggr_correction={"left": 0.02, "right": -0.03})
CASES = {
    "plain": dict(),
    "tta": dict(enable_tta=True),
    "post_process": dict(enable_post_process=True),                                # its threshold is chosen below, on the oracle
    "aggression0": dict(aggression=0),
    "aggr20_tta_post": dict(aggression=20, enable_tta=True, enable_post_process=True, post_process_threshold=0.1),
    "high_end": dict(high_end_process=True),
    "mid_side": dict(params=MID_SIDE, aggression=10),
    "v51": dict(v51=True),
}


def oracle_frame_min(wave, aggression=5):
    """min over (channel, bin) of the mask of one song as inference_vr has it when merge_artifacts looks at it"""
    mp = V.small_params()
    sd = V.make_vr_state(123821, 5, SMALL_CAP)
    X = V.loading_mix(wave, mp)
    seen = {}
    real = V.merge_artifacts

    def spy(mask, thres=0.01, **kw):
        seen["min"] = mask.min(axis=(0, 1)).copy()
        return mask
    V.merge_artifacts = spy
    try:
        aggr = {"value": aggression / 100, "split_bin": mp.param["band"][1]["crop_stop"], "aggr_correction": None}
        V.inference_vr(X, lambda x: V.predict_mask(x, sd, 123821, mp.param["bins"] * 2, 16), 64, 16, 2, aggr, False, False, True, 0.2)
    finally:
        V.merge_artifacts = real
    return seen["min"]


def weight_succeeds(frame_min, thres):
    """merge_artifacts' try block: True when artifact_weight returns a weight, False when it raises"""
    try:
        V.artifact_weight(frame_min, len(frame_min), thres)
        return True
    except Exception:
        return False


def post_process_threshold(waves):
    """A threshold under which the weight function succeeds for at least one song of the pool and raises for another, found on
    the oracle: midway between the songs' largest per-frame mask minima, far from both in units of the engine's error."""
    mins = {id(w): oracle_frame_min(w) for w in waves}
    peaks = sorted(float(m.max()) for m in mins.values())
    gap, thres = max((b - a, (a + b) / 2) for a, b in zip(peaks, peaks[1:]))
    assert gap > 1e-3, peaks
    verdicts = [weight_succeeds(mins[id(w)], thres) for w in waves]
    assert any(verdicts) and not all(verdicts), verdicts
    return thres


@pytest.mark.parametrize("case", list(CASES))
def test_pool_equals_singles(A, g, case):
    """max_batch 3: 1 + 1 + 2 + 6 + 1 = 11 plain patches in passes of 3, 3, 3, 2 -- passes straddle song boundaries and the long
    song spans three passes; with TTA 16 patches in passes of 3 x 5 + 1."""
    kw = dict(CASES[case])
    if kw.pop("v51", False):
        dm = demixer51_at(A, 3)
    else:
        dm = demixer(A, max_batch=3, **kw)
    waves = pool_waves(dm.engine, g["wave"])
    if case == "post_process":
        dm.post_process_threshold = post_process_threshold(waves)
    waves_d = to_dev(waves)
    want = singles(dm, waves_d)
    n0 = dm.engine.counter("vr_net_passes")
    got = dm.separate_stems_many_dev(waves_d)
    plain = sum(t // ROI + 1 for t in FRAMES)
    passes = -(-plain // even_batches(plain, 3))
    if dm.enable_tta:
        passes += -(-(plain + len(FRAMES)) // even_batches(plain + len(FRAMES), 3))
    assert dm.engine.counter("vr_net_passes") - n0 == passes
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a = a.cpu().numpy()
        assert a.shape == b.shape and np.isfinite(b).all()
        assert np.array_equal(a, b), (case, i, rel_rms(a, b))
    assert np.array_equal(got[1].cpu().numpy(), got[4].cpu().numpy())             # the same song at two positions of the pool
    # and the host-array convenience returns what separate_stems returns
    many = dm.separate_stems_many(waves[:2])
    for w, (p, s) in zip(waves[:2], many):
        p1, s1 = dm.separate_stems(w)
        assert np.array_equal(p, p1) and np.array_equal(s, s1)


def test_pool_golden_anchor(A, g):
    """the reference's own stems of vr_small.npz, from a pool in which that song sits between two others"""
    dm = demixer(A, max_batch=3)
    short = pool_waves(dm.engine, g["wave"], (ROI - 1, 2 * ROI + 3))
    out = dm.separate_stems_many([short[0], g["wave"], short[1]])
    p, s = out[1]
    assert p.shape == g["wav_y"].T.shape
    assert rel_rms(p, g["wav_y"].T) < TOL, rel_rms(p, g["wav_y"].T)
    assert rel_rms(s, g["wav_v"].T) < TOL, rel_rms(s, g["wav_v"].T)


@pytest.mark.parametrize("tta", [False, True])
def test_pooling_happened(A, g, tta):
    """Six songs of two patches each at max_batch 4.  Looped: every song runs its 2 patches alone, 6 passes (with TTA 3 more
    patches per song make one more pass each: 12).  Pooled: 12 patches in even_batches(12, 4) = 4 per pass make 3 passes; the TTA
    list of 18 in even_batches(18, 4) = 4 per pass makes 5 more: 8."""
    dm = demixer(A, max_batch=4, enable_tta=tta)
    waves_d = to_dev(pool_waves(dm.engine, g["wave"], (ROI + 3,) * 6))
    assert even_batches(12, 4) == 4 and even_batches(18, 4) == 4 and even_batches(2, 4) == 2 and even_batches(3, 4) == 3
    n0 = dm.engine.counter("vr_net_passes")
    want = singles(dm, waves_d)
    n1 = dm.engine.counter("vr_net_passes")
    got = dm.separate_stems_many_dev(waves_d)
    n2 = dm.engine.counter("vr_net_passes")
    assert (n1 - n0, n2 - n1) == ((12, 8) if tta else (6, 3))
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy(), b)


def test_more_songs_than_one_launch_serves(A, g):
    """cap + 8 songs of one patch each in ONE pass: the gather and the scatter take two launches, the second one with the
    slots counted from its own first song"""
    from audio_separator_amd.engine import VR_POOL_SEGMENTS
    n_songs = VR_POOL_SEGMENTS + 8
    dm = demixer(A, max_batch=n_songs)
    lengths = [length_for(dm.engine, 2 + (i % 5)) + i for i in range(n_songs)]
    waves = [np.ascontiguousarray(g["wave"][:, 300 * i:300 * i + n]) for i, n in enumerate(lengths)]
    assert all(dm.engine.vr_plan(w.shape[1])[0] < ROI for w in waves)
    waves_d = to_dev(waves)
    want = singles(dm, waves_d)
    n0 = dm.engine.counter("vr_net_passes")
    got = dm.separate_stems_many_dev(waves_d)
    assert dm.engine.counter("vr_net_passes") - n0 == 1
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a.cpu().numpy(), b), i


def test_null_outputs(A, g):
    """primary only and secondary only: the stem that is produced equals the one of the both-stems call, the other one's buffer is
    never written"""
    import torch
    dm = demixer(A, max_batch=3, enable_tta=True)
    waves_d = to_dev(pool_waves(dm.engine, g["wave"], (ROI - 1, 2 * ROI + 3, 2)))
    both = [o.cpu().numpy() for o in dm.separate_stems_many_dev(waves_d)]
    for keep in (0, 1):
        outs = [torch.full(b.shape, 7.0, dtype=torch.float32, device="cuda") for b in both]
        songs = [(w.data_ptr(), w.shape[1], o[0].data_ptr() if keep == 0 else 0, o[1].data_ptr() if keep == 1 else 0)
                 for w, o in zip(waves_d, outs)]
        dm.engine.vr_separate_batch_dev(songs, dm.aggressiveness["value"], dm.aggressiveness["split_bin"], **dm._options())
        torch.cuda.synchronize()
        for o, b in zip(outs, both):
            o = o.cpu().numpy()
            assert np.array_equal(o[keep], b[keep]) and (o[1 - keep] == 7.0).all()
    # and through the demixer's keywords
    prim = dm.separate_stems_many_dev(waves_d, want_secondary=False)
    assert all(np.array_equal(p.cpu().numpy()[0], b[0]) for p, b in zip(prim, both))


@pytest.mark.parametrize("bad", ["null_wave", "too_short"])
def test_refusals(A, g, bad):
    """one bad song in the middle of a pool: the call raises, the message names its index, nothing was written"""
    import torch
    dm = demixer(A, max_batch=3)
    waves_d = to_dev(pool_waves(dm.engine, g["wave"], (ROI - 1, 2 * ROI + 3, 2)))
    outs = [torch.full((2, 2, dm.engine.vr_plan(w.shape[1])[1]), 7.0, dtype=torch.float32, device="cuda") for w in waves_d]
    songs = [[w.data_ptr(), w.shape[1], o[0].data_ptr(), o[1].data_ptr()] for w, o in zip(waves_d, outs)]
    if bad == "null_wave":
        songs[1][0] = 0
    else:
        songs[1][1] = 63                                                          # one frame
        assert dm.engine.vr_plan(63)[0] == 1
    with pytest.raises(A.AsxError, match="song 1: " + ("null wave pointer" if bad == "null_wave" else "input too short")):
        dm.engine.vr_separate_batch_dev([tuple(s) for s in songs], dm.aggressiveness["value"], dm.aggressiveness["split_bin"], **dm._options())
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
    # the pool without the bad song goes through on the same engine
    good = dm.separate_stems_many_dev([waves_d[0], waves_d[2]])
    assert all(np.isfinite(o.cpu().numpy()).all() for o in good)


def test_empty_pool(A):
    dm = demixer(A)
    dm.engine.vr_separate_batch_dev([], dm.aggressiveness["value"], dm.aggressiveness["split_bin"])
    assert dm.separate_stems_many_dev([]) == [] and dm.separate_stems_many([]) == []


# ---- files ----------------------------------------------------------------------------------------------------------------
def vr_files(tmp_path, wav):
    """Two PCM_16 files at the rate the device decoder takes (the fixture's top band runs at 8 kHz where the shipped layouts run
    at 44.1 kHz), one PCM_24 file the device decoder is made to decline, one mono file, one file that is not audio."""
    from audio_separator_amd import audio_io
    x, sr = audio_io.read_wav(wav)
    assert sr == 8000 and x.shape[0] == 2
    n = x.shape[1]
    srcs = []
    for i, (a, subtype) in enumerate([(x[:, :n // 4], "PCM_16"), (x[:, n // 5: n // 5 + 3001], "PCM_16"), (x[:, n // 2: n // 2 + n // 3], "PCM_24"),
                                      (x[:1, :5000], "PCM_16")]):
        path = str(tmp_path / f"song{i}.wav")
        audio_io.write_wav(path, np.ascontiguousarray(a.T), sr, subtype)
        srcs.append(path)
    assert audio_io.wav_info(srcs[3])["channels"] == 1
    bad = str(tmp_path / "broken.wav")
    with open(bad, "wb") as f:
        f.write(b"not a wave file")
    return srcs[:3] + [bad] + srcs[3:]


@pytest.mark.parametrize("tag", ["vr_plain", "vr_tta_single"])
def test_separate_many_files(tag, tmp_path, monkeypatch):
    """separate_many over device-decoded, host-decoded, mono and unreadable files: the names and the bytes of separate(path) per
    file, in order; the unreadable one fails alone.  vr_tta_single: output_single_stem, TTA, post-processing, high_end_process."""
    from audio_separator_amd import audio_io
    case = [c for c in SC.cases("vr", str(tmp_path)) if c[0] == tag][0]
    _, cls, common, arch, wav, _ = case
    srcs = vr_files(tmp_path, wav)
    klass = SC.plugin_class(cls)
    real, decoded = klass._device_mix, []

    def device_mix(self, path, check_silent=True):
        assert check_silent is False                                              # VR does not refuse silent input
        mix = None if path == srcs[2] else real(self, path, check_silent)
        decoded.append((os.path.basename(path), mix is not None))
        return mix
    monkeypatch.setattr(klass, "_device_mix", device_mix)

    def no_prepare_mix(self, mix):
        raise AssertionError("the VR plugin never calls prepare_mix")
    monkeypatch.setattr(klass, "prepare_mix", no_prepare_mix)
    expect_decoded = [("song0.wav", True), ("song1.wav", True), ("song2.wav", False), ("broken.wav", False), ("song3.wav", True)]
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    inst = klass(common_config=dict(common, output_dir=one_dir), arch_config=arch)
    want = []
    for path in srcs:
        try:
            want.append(inst.separate(path, None))
        except Exception:
            want.append([])
        inst.clear_gpu_cache()
        inst.clear_file_specific_paths()
    assert decoded == expect_decoded
    del decoded[:]
    inst = klass(common_config=dict(common, output_dir=many_dir), arch_config=arch)
    got = inst.separate_many(srcs)
    assert decoded == expect_decoded
    assert inst.input_subtype is None
    assert got == want and got[3] == [] and list(inst.batch_errors) == [3]
    per_file = 1 if common.get("output_single_stem") else 2
    assert all(len(names) == per_file for i, names in enumerate(got) if i != 3), got
    for names in want:
        for name in names:
            assert filecmp.cmp(os.path.join(one_dir, name), os.path.join(many_dir, name), shallow=False), name
    assert audio_io.info(os.path.join(many_dir, want[2][0]))["subtype"] == "PCM_24"
    assert audio_io.info(os.path.join(many_dir, want[0][0]))["subtype"] == "PCM_16"


def test_separate_many_short_file_fails_alone(tmp_path):
    """a file with fewer than two frames is found while loading (engine.vr_plan) and never reaches the pooled call"""
    from audio_separator_amd import audio_io
    _, cls, common, arch, wav, _ = SC.cases("vr", str(tmp_path))[0]
    x, sr = audio_io.read_wav(wav)
    paths = []
    for i, n in enumerate((4000, 40, 3000)):
        paths.append(str(tmp_path / f"s{i}.wav"))
        audio_io.write_wav(paths[-1], np.ascontiguousarray(x[:, :n].T), sr, "PCM_16")
    inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=str(tmp_path / "out")), arch_config=arch)
    got = inst.separate_many(paths)
    assert [len(names) for names in got] == [2, 0, 2] and list(inst.batch_errors) == [1]
    assert "too short" in str(inst.batch_errors[1])
