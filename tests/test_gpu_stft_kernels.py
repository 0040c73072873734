"""Every STFT / iSTFT launch against a float64 DFT, one launch at a time through asx_op_stft / asx_op_istft / asx_op_ht_spec /
asx_op_ht_ispec (include/asx.h): the generic LDS Stockham family (stft_kernel, stft_pool_kernel, istft_kernel, ola_kernel of
csrc/kernels_fft.h) at one plan per radix mix and in its three layouts, the 6144 / 1024 fast path (stft3 / stft3p and their pool twins,
istft3 / istft3p, seam3 of csrc/kernels_fft3.h) and the Demucs family (ht_stft_kernel, ht_istft_kernel, ht_ola_kernel of csrc/kernels_ht.h).
The hooks go through the launch helpers and argument builders the nets use (csrc/engine_mdx.h, engine_v3.h, engine_rof.h, engine_ht.h).

Error measure (tests/stft_ref.py): forward, the worst element of |kernel - f64| / P_t, P_t the largest |X64| over bins 0 .. n/2 of the
element's frame before cropping or zeroing; inverse, the worst sample of |kernel - f64| / s_j, s_j = (sum_t peak_t |w[m - t hop]|) / env[m]
with peak_t the largest |irfft64| of frame t before the window (times the chunk window; plus |time branch| for Demucs).  NaN counts as
infinite.  Frames whose float64 spectrum is identically zero and samples with s_j = 0 must come back as exact zeros, asserted apart.
Bar: 8 x max(e32, 2^-23), e32 the same measure of torch's fp32 rfft / irfft evaluation of the same input on the CPU at run time; the
factor 8 is that of test_gpu_gconv.py and test_gpu_lstm_kernels.py.  Nothing in the bar comes from the kernels' output.
Every case goes in with a NaN-filled output (what the launch does not own -- batch-stride gaps -- must come back bit for bit), asserts
`resolved`, runs twice and must repeat bit for bit; cases of the fast path run once more on an engine of the generic kernels.

Measured on an MI355X, the worst measured / bar per kernel over the cases below (all pass; the bar is 1.000; errors are 1.4e-7 ..
3.0e-7 of the scale, level with torch's fp32 evaluation):
  stft_kernel        0.180 (fwd-plan-160-16.5)        stft_pool_kernel     0.129 (fwd3p-pool-T6-F3072 on the generic engine)
  stft3_kernel       0.159 (fwd3-song-T6-F3072)       stft3_pool_kernel    0.146 (fwd3-pool-T16-F3072)
  stft3p_kernel      0.173 (fwd3p-song-T6-F3072)      stft3p_pool_kernel   0.121 (fwd3p-pool-T6-F3072)
  istft + ola        0.178 (inv-dimf-half)            istft3 (+ seam3)     0.146 (inv3-combine)
  istft3p (+ seam3)  0.155 (inv3p-T6)                 ht_stft_kernel       0.153 (ht-spec-1024-L3)
  ht_istft + ht_ola  0.136 (ht-ispec-1024-L2000)
No element without a scale came back other than an exact zero.
"""
import contextlib
import os

import numpy as np
import pytest

from tests import stft_cases as K
from tests import stft_ref as R

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def engine(c, extra_env=None):
    """an engine of the case's geometry, created under the case's environment (the per-engine knobs are read at creation)"""
    import audio_separator_amd as A
    env = dict(c.get("env", {}), **(extra_env or {}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = A.Engine(A.MDXConfig(n_fft=c["n_fft"], hop_length=c["hop"], dim_f=c["dim_f"], segment_size=K.segment_size(c),
                                 win_length=c["win_length"]))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        if c["window"] == "hamming":
            e.set_stft_window(R.hamming_table(c["n_fft"]))
        yield e
    finally:
        e.close()


@contextlib.contextmanager
def stop_on_hip_error():
    """a failed HIP call (ASX_ERR_HIP = 2: a launch error or a fault) ends the session: nothing more is started on that device"""
    from audio_separator_amd.engine import AsxError
    try:
        yield
    except AsxError as e:
        if str(e).startswith("asx error 2"):
            pytest.exit(f"HIP error, stopping: {e}", returncode=3)
        raise


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def report(c, ran, err, e32, zero_bad):
    bar = R.bar(e32)
    print(f"{c['name']} [{ran[0]}, {ran[1]} seam launches]: err {err:.3e} e32 {e32:.3e} bar {bar:.3e} measured / bar {err / bar:.3f}; "
          f"{zero_bad} scale-less elements not exact zeros")
    assert zero_bad == 0, f"{c['name']}: {zero_bad} elements without a scale are not exact zeros"
    assert err <= bar, f"{c['name']}: off by {err:.3e} of its scale, plain fp32 by {e32:.3e} (bar {bar:.3e})"


def run_forward(c, d, eng, expect):
    spec0 = np.full(d["size"], np.nan, np.float32)
    spec, ran = eng.op_stft(d["wave"], spec0, **d["desc"])
    spec2, ran2 = eng.op_stft(d["wave"], spec0, **d["desc"])
    assert ran == ran2 and same_bits(spec, spec2), f"{c['name']}: two runs differ"
    assert ran == expect, f"{c['name']}: ran {ran}, expected {expect}"
    own = np.zeros(d["size"], bool)
    own[d["idx"].reshape(-1)] = True
    assert same_bits(spec[~own], spec0[~own]), f"{c['name']}: wrote outside its planes"
    err, zero_bad = R.forward_measure(R.as_complex(spec, d["idx"]), d["X"], d["P"], c["dim_f"], c["zero_low"])
    report(c, ran, err, d["e32"], zero_bad)


def run_inverse(c, d, eng, expect):
    wave0 = np.full(d["out"].shape, np.nan, np.float32)
    wave, ran = eng.op_istft(d["spec"], wave0, mask=d["mask"], **d["desc"])
    wave2, ran2 = eng.op_istft(d["spec"], wave0, mask=d["mask"], **d["desc"])
    assert ran == ran2 and same_bits(wave, wave2), f"{c['name']}: two runs differ"
    assert ran == expect, f"{c['name']}: ran {ran}, expected {expect}"
    err, zero_bad = R.measure(wave, d["out"], d["s"])
    report(c, ran, err, d["e32"], zero_bad)


@pytest.mark.parametrize("name", [c["name"] for c in K.FWD])
def test_stft_vs_float64(name):
    c, d = K.BY_NAME[name], K.build(name)
    with stop_on_hip_error(), engine(c) as eng:
        run_forward(c, d, eng, c["expect"])
    if c["generic"]:
        with stop_on_hip_error(), engine(c, {"ASX_FFT3": "0"}) as eng:
            run_forward(c, d, eng, ("stft_pool" if c["mode"] == "pool" else "stft", 0))


@pytest.mark.parametrize("name", [c["name"] for c in K.INV])
def test_istft_vs_float64(name):
    c, d = K.BY_NAME[name], K.build(name)
    with stop_on_hip_error(), engine(c) as eng:
        run_inverse(c, d, eng, c["expect"])
    if c["generic"]:
        with stop_on_hip_error(), engine(c, {"ASX_FFT3": "0"}) as eng:
            run_inverse(c, d, eng, ("istft+ola", 0))


@pytest.fixture(scope="module")
def ht_eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


@pytest.mark.parametrize("name", [c["name"] for c in K.HT if c["dir"] == "ht_spec"])
def test_ht_spec_vs_float64(ht_eng, name):
    c, d = K.BY_NAME[name], K.build(name)
    with stop_on_hip_error():
        spec = ht_eng.op_ht_spec(c["nfft"], d["seg"], d["el"], d["lv"])
        spec2 = ht_eng.op_ht_spec(c["nfft"], d["seg"], d["el"], d["lv"])
    assert same_bits(spec, spec2), f"{name}: two runs differ"
    got = (spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)).transpose(0, 3, 1, 2)      # [B, ch, T, F]
    err, zero_bad = R.forward_measure(got, d["X"], d["P"], c["nfft"] // 2)
    report(c, ("ht_stft", 0), err, d["e32"], zero_bad)


@pytest.mark.parametrize("name", [c["name"] for c in K.HT if c["dir"] == "ht_ispec"])
def test_ht_ispec_vs_float64(ht_eng, name):
    c, d = K.BY_NAME[name], K.build(name)
    with stop_on_hip_error():
        out = ht_eng.op_ht_ispec(c["nfft"], d["x"], d["acc_f"], d["n_stat"], d["xt"], d["acc_t"])
        out2 = ht_eng.op_ht_ispec(c["nfft"], d["x"], d["acc_f"], d["n_stat"], d["xt"], d["acc_t"])
    assert same_bits(out, out2), f"{name}: two runs differ"
    err, zero_bad = R.measure(out, d["out"], d["s"])
    report(c, ("ht_istft+ht_ola", 0), err, d["e32"], zero_bad)
