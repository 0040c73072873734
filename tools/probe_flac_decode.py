#!/usr/bin/env python3
"""What a FLAC input costs beside a WAV input of the same samples: ``MDXSeparator.separate`` (the HQ_3 geometry of bench.py's ``file_level``
key) on a 4-minute 44.1 kHz stereo song in tmpfs, once from the PCM16 WAV and once from the FLAC file the device encoder makes of it
(block 4096).  Per input: the median over 5 calls after one warm-up of the call's wall time and of the ``file_timings`` phases -- ``read``,
``h2d_decode`` (WAV) or ``flac_decode`` (FLAC), ``demix`` and the rest -- and the edge's share of the wall time.  Then the decoder alone on
the audio part already in HBM: the three launches' times from the engine profile (sync, frame, finish) and the wall time of the two calls.
One JSON line.

    python tools/probe_flac_decode.py [--seconds 240]
"""
import argparse
import json
import logging
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_separator_amd as A  # noqa: E402
from audio_separator_amd import audio_io  # noqa: E402
from audio_separator_amd.architectures.mdx_separator import MDXSeparator  # noqa: E402
from oracle import mdx_oracle as O  # noqa: E402

SR = 44100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    args = ap.parse_args()
    import torch
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_flacdec_", dir=base)
    try:
        n = int(SR * args.seconds)
        wav, flac = os.path.join(tmp, "song.wav"), os.path.join(tmp, "song.flac")
        audio_io.write_wav(wav, np.ascontiguousarray(O.synth_mix(n, seed=0).T), SR, "PCM_16")
        x, _ = audio_io.read_wav(wav)
        pcm = np.ascontiguousarray(np.rint(x.T.astype(np.float64) * 32768.0), np.int16)
        sd = O.make_convtdf_state(O.NetDims(), seed=0)
        log = logging.getLogger("probe.flacdec")
        log.setLevel(logging.ERROR)
        common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                  "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": "UVR-MDX-NET-Inst_HQ_3", "model_path": None,
                  "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                 "primary_stem": "Instrumental"},
                  "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, "out"), "normalization_threshold": 0.9,
                  "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False, "sample_rate": SR,
                  "use_soundfile": False, "asx_state_dict": sd, "asx_net_config": A.NetConfig(), "asx_profile_file": True}
        arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
        sep = MDXSeparator(common, arch)
        eng = sep.engine
        frames, sizes = eng.flac_encode(pcm, SR, 16, 4096)
        audio_io.write_flac(flac, frames, sizes, SR, 16, n)
        out = {"what": f"MDXSeparator.separate of a {args.seconds:g}-s 44.1 kHz stereo song on tmpfs, PCM16 WAV against 16-bit FLAC input; "
                       f"medians of 5 calls after a warm-up",
               "wav_bytes": os.path.getsize(wav), "flac_bytes": os.path.getsize(flac), "n_frames": int(sizes.size)}
        for key, path, edge in (("WAV", wav, ("read", "h2d_decode")), ("FLAC", flac, ("read", "flac_decode"))):
            walls, phases = [], {}
            for call in range(6):
                t0 = time.perf_counter()
                sep.separate(path)
                if call:
                    walls.append(time.perf_counter() - t0)
                    for k, v in sep.file_timings.items():
                        phases.setdefault(k, []).append(v)
                sep.clear_gpu_cache()
                sep.clear_file_specific_paths()
            med = {k: statistics.median(v) for k, v in phases.items()}
            wall = statistics.median(walls)
            out[key] = {"wall_ms": round(wall * 1e3, 2), "phases_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
                        "edge_ms": round(sum(med.get(k, 0.0) for k in edge) * 1e3, 3),
                        "edge_share_of_wall": round(sum(med.get(k, 0.0) for k in edge) / wall, 4)}
        # the decoder alone, the audio part in HBM
        info = audio_io.flac_stream(flac)
        with open(flac, "rb") as f:
            f.seek(info["audio_offset"])
            raw = torch.frombuffer(bytearray(f.read()), dtype=torch.uint8).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        calls = []
        for it in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found = eng.flac_decode_scan_dev(raw.data_ptr(), raw.numel(), info, stream=stream)
            t1 = time.perf_counter()
            mix = torch.empty((2, found["n_samples"]), dtype=torch.float32, device="cuda")
            eng.flac_decode_finish_dev(mix.data_ptr(), found["n_samples"], stream=stream)
            t2 = time.perf_counter()
            if it:
                calls.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        eng.profile_enable(True)
        found = eng.flac_decode_scan_dev(raw.data_ptr(), raw.numel(), info, stream=stream)
        eng.flac_decode_finish_dev(mix.data_ptr(), found["n_samples"], stream=stream)
        launches = [ms for cls, ms, _, _ in eng.profile_launches() if cls == "misc"][-3:]
        eng.profile_enable(False)
        plan = eng.flac_decode_plan(raw.numel(), 2, 16, info["max_blocksize"], info["max_framesize"])
        out["decode_alone"] = {"scan_call_ms": round(statistics.median(c[0] for c in calls), 3),
                               "finish_call_ms": round(statistics.median(c[1] for c in calls), 3),
                               "kernel_ms": dict(zip(("flac_sync_kernel", "flac_frame_kernel", "flac_finish_kernel"), (round(v, 3) for v in launches))),
                               "found": found, "audio_bytes": raw.numel(), "max_candidates": plan["max_candidates"],
                               "exact": bool(torch.equal(mix, torch.from_numpy(pcm.T.astype(np.float32) / 32768.0).cuda()))}
        eng.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
