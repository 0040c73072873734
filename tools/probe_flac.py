#!/usr/bin/env python3
"""What FLAC output costs beside WAV output: ``MDXSeparator.separate(song.wav)`` (the HQ_3 geometry of bench.py's ``file_level`` key) on a
4-minute PCM16 WAV in tmpfs, two stem files, once with ``output_format`` WAV and once with FLAC on the same tree; then the encoder on its
own for one stem's int16 already in HBM (hipEvent time of the three launches, wall time of the call with its synchronise and of bringing
the frames back), at 16 and 24 bits.  One JSON line.

    python tools/probe_flac.py [--seconds 240]
"""
import argparse
import json
import logging
import os
import shutil
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
    tmp = tempfile.mkdtemp(prefix="asx_flac_", dir=base)
    try:
        n = int(SR * args.seconds)
        wav = os.path.join(tmp, "song.wav")
        audio_io.write_wav(wav, np.ascontiguousarray(O.synth_mix(n, seed=0).T), SR, "PCM_16")
        sd = O.make_convtdf_state(O.NetDims(), seed=0)
        log = logging.getLogger("probe.flac")
        log.setLevel(logging.ERROR)
        out = {"what": f"MDXSeparator.separate({args.seconds:g}-s PCM16 WAV on tmpfs) -> 2 stem files, WAV against FLAC output"}
        for fmt in ("WAV", "FLAC"):
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": "UVR-MDX-NET-Inst_HQ_3", "model_path": None,
                      "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                     "primary_stem": "Instrumental"},
                      "output_format": fmt, "output_bitrate": None, "output_dir": os.path.join(tmp, fmt), "normalization_threshold": 0.9,
                      "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False, "sample_rate": SR,
                      "use_soundfile": False, "asx_state_dict": sd, "asx_net_config": A.NetConfig(), "asx_profile_file": True}
            arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
            sep = MDXSeparator(common, arch)
            walls, phases = [], {}
            for call in range(4):
                t0 = time.perf_counter()
                files = sep.separate(wav)
                if call:                                        # the first call warms workspaces, pinned staging and the page cache
                    walls.append(time.perf_counter() - t0)
                    for k, v in sep.file_timings.items():
                        phases[k] = phases.get(k, 0.0) + v
                sep.clear_gpu_cache()
                sep.clear_file_specific_paths()
            out[fmt] = {"wall_ms": round(sum(walls) / len(walls) * 1e3, 2), "rtf": round(args.seconds * len(walls) / sum(walls), 1),
                        "phases_ms": {k: round(v / len(walls) * 1e3, 2) for k, v in phases.items()},
                        "file_bytes": [os.path.getsize(os.path.join(common["output_dir"], f)) for f in files], "how": sep.last_write_path}
            if fmt == "FLAC":
                eng = sep.engine
                x, _ = audio_io.read_wav(os.path.join(common["output_dir"], "..", "WAV", os.path.splitext(files[0])[0] + ".wav"))
                pcm = torch.from_numpy(np.ascontiguousarray(np.rint(x.T * 32768.0).astype(np.int16))).cuda()
                enc = {}
                for bits in (16, 24):
                    plan = eng.flac_plan(n, 2, bits, 4096)
                    buf = torch.empty(plan["max_bytes"], dtype=torch.uint8, device="cuda")
                    sizes = torch.empty(plan["n_blocks"], dtype=torch.int32, device="cuda")
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    dev_ms, call_ms, back_ms = [], [], []
                    for it in range(4):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        a.record()
                        total = eng.flac_encode_dev(pcm.data_ptr(), n, SR, bits, 4096, buf.data_ptr(), plan["max_bytes"], sizes.data_ptr(),
                                                    stream=torch.cuda.current_stream().cuda_stream)
                        b.record()
                        t1 = time.perf_counter()
                        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)      # as the writer brings them back
                        host.copy_(buf[:total], non_blocking=True)
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        if it:
                            dev_ms.append(a.elapsed_time(b))
                            call_ms.append((t1 - t0) * 1e3)
                            back_ms.append((t2 - t1) * 1e3)
                    # lane 0's clock stamps of a profiled encode: the share of a block's time spent in its CRC-16 phases
                    c0 = (eng.counter("flac_block_cycles"), eng.counter("flac_crc16_cycles"))
                    eng.profile_enable(True)
                    eng.flac_encode_dev(pcm.data_ptr(), n, SR, bits, 4096, buf.data_ptr(), plan["max_bytes"], sizes.data_ptr(),
                                        stream=torch.cuda.current_stream().cuda_stream)
                    eng.profile_enable(False)
                    blk_cyc, crc_cyc = eng.counter("flac_block_cycles") - c0[0], eng.counter("flac_crc16_cycles") - c0[1]
                    enc[f"crc16_share_{bits}"] = round(crc_cyc / max(blk_cyc, 1), 4)
                    enc[str(bits)] = {"device_ms": round(min(dev_ms), 3), "call_ms": round(min(call_ms), 3), "frames_d2h_ms": round(min(back_ms), 3),
                                      "frames_bytes": int(total), "pcm16_bytes": 4 * n, "n_blocks": plan["n_blocks"],
                                      "scratch_bytes": plan["scratch_bytes"], "frames_crc": int(host.numpy().astype(np.uint64).sum())}
                out["encode_one_stem"] = enc
            sep.engine.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
