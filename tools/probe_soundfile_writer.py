#!/usr/bin/env python3
"""What ``use_soundfile=True`` costs at the file level: ``MDXSeparator.separate(song.wav)`` (the HQ_3 geometry of bench.py's ``file_level`` key)
on a 4-minute WAV in tmpfs, two stem files, soundfile absent, for the inputs PCM_16, PCM_24 and FLOAT with WAV output and PCM_24 with a
``.flac`` name.  Per row: the file-to-files wall time of five calls after a warm-up call (median, and the spread max - min), the phases the
class records, how the stems reached their files, and the size of the files against the 16-byte-per-frame float stems.  Where the engine
has it, the sample-format encoder on its own for one stem in HBM (hipEvent time, GB/s of input + output).  One JSON line.

``--tree`` names the checkout whose package is measured (default: the one this file is in), so that one job can run the same probe on two
commits, one after the other on the same card:

    python tools/probe_soundfile_writer.py [--seconds 240] [--tree /path/to/another/checkout]
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

SR = 44100
ROWS = (("PCM_16", "WAV"), ("PCM_24", "WAV"), ("FLOAT", "WAV"), ("PCM_24", "FLAC"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from oracle import mdx_oracle as O

    real = audio_io._optional
    audio_io._optional = lambda name: None if name == "soundfile" else real(name)      # the rows are about the built-in writer
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_sfw_", dir=base)
    try:
        n = int(SR * args.seconds)
        mix = np.ascontiguousarray(O.synth_mix(n, seed=0).T)
        sd = O.make_convtdf_state(O.NetDims(), seed=0)
        log = logging.getLogger("probe.soundfile_writer")
        log.setLevel(logging.CRITICAL)
        out = {"what": f"MDXSeparator.separate({args.seconds:g}-s WAV on tmpfs, use_soundfile=True, soundfile absent) -> 2 stem files",
               "tree": os.path.abspath(args.tree), "device_encoder": hasattr(A.Engine, "pcm_encode_dev"), "rows": {}}
        sep = None
        for subtype, fmt in ROWS:
            wav = os.path.join(tmp, f"song_{subtype}.wav")
            if not os.path.exists(wav):
                audio_io.write_wav(wav, mix, SR, subtype)
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": "UVR-MDX-NET-Inst_HQ_3", "model_path": None,
                      "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                     "primary_stem": "Instrumental"},
                      "output_format": fmt, "output_bitrate": None, "output_dir": os.path.join(tmp, f"{subtype}_{fmt}"),
                      "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                      "sample_rate": SR, "use_soundfile": True, "asx_state_dict": sd, "asx_net_config": A.NetConfig(), "asx_profile_file": True}
            arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
            sep = MDXSeparator(common, arch)
            walls, phases = [], {}
            for call in range(args.calls + 1):
                t0 = time.perf_counter()
                files = sep.separate(wav)
                if call:                                        # the first call warms workspaces, pinned staging and the page cache
                    walls.append(time.perf_counter() - t0)
                    for k, v in sep.file_timings.items():
                        phases[k] = phases.get(k, 0.0) + v
                sep.clear_gpu_cache()
                sep.clear_file_specific_paths()
            paths = [os.path.join(common["output_dir"], f) for f in files]
            heads = []
            for p in paths:
                with open(p, "rb") as f:
                    heads.append(f.read(4).decode("latin-1"))
            sizes = [os.path.getsize(p) for p in paths]
            out["rows"][f"{subtype}->{fmt}"] = {
                "wall_ms_median": round(statistics.median(walls) * 1e3, 2), "wall_ms_spread": round((max(walls) - min(walls)) * 1e3, 2),
                "wall_ms": [round(w * 1e3, 2) for w in walls], "phases_ms": {k: round(v / len(walls) * 1e3, 2) for k, v in phases.items()},
                "how": getattr(sep, "last_write_path", None), "file_bytes": sizes, "file_magic": heads,
                "bytes_per_float_stem_byte": round(sum(sizes) / (len(sizes) * 8.0 * n), 4)}
            if (subtype, fmt) != ROWS[-1]:
                sep.engine.close()
        eng = sep.engine
        if out["device_encoder"]:
            # the encoder alone: one [n, 2] stem in HBM -> the body of its data chunk, the launches timed by hipEvents
            stem = torch.from_numpy((0.5 * mix).astype(np.float32)).cuda()
            body = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
            enc = {}
            for subtype, frame_bytes in (("PCM_16", 4), ("PCM_24", 6), ("PCM_32", 8), ("FLOAT", 8)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ms = []
                for it in range(6):
                    torch.cuda.synchronize()
                    a.record()
                    eng.pcm_encode_dev(stem.data_ptr(), n, "rows", 0.9, 0.0, subtype, body.data_ptr(),
                                       stream=torch.cuda.current_stream().cuda_stream, want_peak=False)
                    b.record()
                    torch.cuda.synchronize()
                    if it:
                        ms.append(a.elapsed_time(b))
                moved = n * (8 + 8 + frame_bytes)              # the peak pass reads the stem once, the encoder reads it again and writes the body
                enc[subtype] = {"device_ms": round(statistics.median(ms), 4), "gb_per_s": round(moved / (statistics.median(ms) * 1e-3) / 1e9, 1)}
            out["pcm_encode_one_stem"] = enc
        eng.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
