"""The FLAC encoder for int32 samples of 16 or 24 real bits on the device (asx_flac_encode_pcm / asx_flac_encode_pcm_dev: flac_encode_kernel<true>
of csrc/kernels_flac.h) on the contents of the host-compiled kernel's test (tests/flac_wide_cases.py): decoded by tests/flac_ref.py, which
verifies every CRC, the samples must be exactly what went in.  What the host build cannot show is here: barriers, LDS atomics, the launch."""
import numpy as np
import pytest

from tests import flac_wide_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(), device=0)
    yield e
    e.close()


@pytest.mark.parametrize("name,bits", [(n, b) for n, b, _ in W.CASES])
def test_exact_round_trip(eng, name, bits):
    pcm = next(p for n, b, p in W.CASES if n == name and b == bits)
    plan = eng.flac_plan_pcm(pcm.shape[0], 2, bits, 4096)
    frames, sizes = eng.flac_encode_pcm(pcm, W.RATE, bits, 4096)
    assert sizes.shape == (plan["n_blocks"],) and int(sizes.sum()) == frames.size <= plan["max_bytes"]
    assert int(sizes.max()) <= plan["frame_stride"]
    decoded = W.check_stream(frames.tobytes(), sizes, pcm, bits, 4096)
    subs = [s for d in decoded for s in d["subframes"]]
    assert all(s["wasted"] == 0 for s in subs)
    kinds = {s["type"] for s in subs}
    if name in ("silence", "constant_dc", "constant_-3"):
        assert kinds == {"CONSTANT"}
    if name == "white_noise_full_scale":
        assert kinds == {"VERBATIM"}
    if name == "noise_2^19":
        assert any(s.get("method") == 1 and max(s["params"]) > 14 for s in subs)
    if name == "sine_-60dbfs":
        assert kinds <= {"FIXED", "LPC"} and all(s["method"] == 0 for s in subs)
        assert frames.size < sum((2 * (8 + 24 * d["blocksize"]) + 7) // 8 for d in decoded)


def test_two_encodes_are_byte_identical(eng):
    for name in ("noise_2^19", "sine_-60dbfs", "square_near_nyquist_full_scale"):
        pcm = W.CONTENTS24[name]
        a, sa = eng.flac_encode_pcm(pcm, W.RATE, 24, 4096)
        b, sb = eng.flac_encode_pcm(pcm, W.RATE, 24, 4096)
        assert np.array_equal(a, b) and np.array_equal(sa, sb) and int(sa.sum()) == a.size


def test_other_block_sizes_and_rates(eng):
    for name in ("noise_2^19", "left_only"):
        pcm = W.CONTENTS24[name][:2 * 4608 + 5]
        for block, rate in ((4608, 48000), (16, 12345), (1000, 96000)):
            frames, sizes = eng.flac_encode_pcm(pcm, rate, 24, block)
            W.check_stream(frames.tobytes(), sizes, pcm, 24, block, rate)


def test_refusals(eng):
    import audio_separator_amd as A
    import torch
    with pytest.raises(A.AsxError, match="outside 24 bits"):
        eng.flac_encode_pcm(np.array([[0, 0], [1 << 23, 0]], np.int32), W.RATE, 24)
    with pytest.raises(A.AsxError, match="outside 16 bits"):
        eng.flac_encode_pcm(np.array([[-32769, 0]], np.int32), W.RATE, 16)
    with pytest.raises(ValueError, match="int32"):
        eng.flac_encode_pcm(np.zeros((4, 2), np.int16), W.RATE, 16)
    pcm = torch.zeros((100, 2), dtype=torch.int32, device="cuda")
    out = torch.empty(16, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(1, dtype=torch.int32, device="cuda")
    with pytest.raises(A.AsxError, match="out_capacity"):
        eng.flac_encode_pcm_dev(pcm.data_ptr(), 100, W.RATE, 24, 4096, out.data_ptr(), 16, sizes.data_ptr())
    with pytest.raises(A.AsxError, match="bits per sample"):
        eng.flac_encode_pcm_dev(pcm.data_ptr(), 100, W.RATE, 20, 4096, out.data_ptr(), 16, sizes.data_ptr())
