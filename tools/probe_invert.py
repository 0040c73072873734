#!/usr/bin/env python3
"""What ``invert_using_spec=True`` costs at the file level: ``MDXSeparator.separate(song.wav)`` (the HQ_3 geometry of bench.py's
``file_level`` key) on a 4-minute PCM_16 WAV in tmpfs, two stem files, with the option off and on.  Per row: the file-to-files wall time
of five calls after a warm-up call (median, and the spread max - min), the phases the class records and whether the file was decoded on
the device.  Then an ``EnsembleSeparator`` of two such members (option on, avg_wave) on its default path and with ``via_files=True``,
with the path each input took.  One JSON line.

``--tree`` names the checkout whose package is measured (default: the one this file is in), so that one job can run the same probe on two
commits, alternating on the same card:

    python tools/probe_invert.py [--seconds 240] [--tree /path/to/another/checkout] [--label "parent commit"] [--no-ensemble]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-ensemble", action="store_true")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--tree", default=here)
    ap.add_argument("--label", default=None, help="what the record calls the measured tree (default: its path)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.append(here)                                      # the synthetic mix and weights, where the measured tree is only the package
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from oracle import mdx_oracle as O

    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_inv_", dir=base)
    try:
        n = int(SR * args.seconds)
        wav = os.path.join(tmp, "song.wav")
        audio_io.write_wav(wav, np.ascontiguousarray(O.synth_mix(n, seed=0).T), SR, "PCM_16")
        sd = O.make_convtdf_state(O.NetDims(), seed=0)
        log = logging.getLogger("probe.invert")
        log.setLevel(logging.CRITICAL)

        def member(out_dir, invert):
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": "UVR-MDX-NET-Inst_HQ_3", "model_path": None,
                      "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                     "primary_stem": "Instrumental"},
                      "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, out_dir),
                      "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": invert,
                      "sample_rate": SR, "use_soundfile": False, "asx_state_dict": sd, "asx_net_config": A.NetConfig(), "asx_profile_file": True}
            arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
            return MDXSeparator(common, arch)

        def timed(call, after):
            walls = []
            for i in range(args.calls + 1):
                t0 = time.perf_counter()
                call()
                if i:                                           # the first call warms workspaces, pinned staging and the page cache
                    walls.append(time.perf_counter() - t0)
                    after(True)
                else:
                    after(False)
            return {"wall_ms_median": round(statistics.median(walls) * 1e3, 2), "wall_ms_spread": round((max(walls) - min(walls)) * 1e3, 2),
                    "wall_ms": [round(w * 1e3, 2) for w in walls]}

        out = {"what": f"MDXSeparator.separate({args.seconds:g}-s PCM_16 WAV on tmpfs) -> 2 stem files", "tree": args.label or os.path.abspath(args.tree),
               "device_invert": hasattr(A.Engine, "invert_stem_dev"), "rows": {}}
        for invert in (False, True):
            sep = member(f"single_{int(invert)}", invert)
            phases = {}

            def after(counted, sep=sep, phases=phases):
                if counted:
                    for k, v in sep.file_timings.items():
                        phases[k] = phases.get(k, 0.0) + v
                sep.clear_gpu_cache()
                sep.clear_file_specific_paths()
            row = timed(lambda sep=sep: sep.separate(wav), after)
            row["phases_ms"] = {k: round(v / args.calls * 1e3, 2) for k, v in phases.items()}
            row["decoded_on_device"] = "h2d_decode" in phases
            out["rows"][f"invert_using_spec={invert}"] = row
            sep.engine.close()
        if not args.no_ensemble:
            members = [member("member_0", True), member("member_1", True)]
            for via_files in (False, True):
                ens = A.EnsembleSeparator(members, "avg_wave", None, via_files=via_files, logger=log)
                ens.output_dir = os.path.join(tmp, f"ensemble_{int(via_files)}")
                taken = []
                row = timed(lambda ens=ens: ens.separate(wav), lambda counted, ens=ens: taken.append(ens.last_path_taken))
                row["path_taken"] = sorted(set(taken))
                out["rows"][f"ensemble of 2, invert_using_spec=True, via_files={via_files}"] = row
            for m in members:
                m.engine.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
