#!/usr/bin/env python3
"""What ``pitch_shift`` costs at the file level on the MDXC plugin: ``MDXCSeparator.separate(song.wav)`` on a 4-minute PCM_16 WAV in tmpfs,
two stem files, and ``separate_many`` over eight such files, on the MDX23C and the BS-Roformer ep_317 layouts (synthetic weights, the
geometries of tools/bench_mdxc_batch.py), with ``pitch_shift`` 0 and 2.  Per row: the files-to-files wall time of five calls after a
warm-up call (median, and the spread max - min), the phases the class records for the single file, and whether the files were decoded on
the device.  One JSON line.

``--tree`` names the checkout whose package is measured (default: the one this file is in), so that one job can run the same probe on two
commits, alternating on the same card:

    python tools/probe_pitch.py [--nets mdx23c,rof] [--seconds 240] [--files 8] [--tree /path/to/another/checkout] [--label "parent commit"]
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
NETS = {"mdx23c": "MDX23C layout, overlap 2, 8 chunks per pass", "rof": "BS-Roformer ep_317 layout, overlap 8 (step = chunk), 16 chunks per pass"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="mdx23c,rof")
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shifts", default="0,2")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--tree", default=here)
    ap.add_argument("--label", default=None, help="what the record calls the measured tree (default: its path)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.append(here)                                      # the synthetic mix and weights, where the measured tree is only the package
    import torch
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdxc_separator import MDXCSeparator
    from tools.bench_mdxc_batch import make_model
    from tools.bench_siblings import synth

    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_pitch_", dir=base)
    try:
        n = int(SR * args.seconds)
        first = synth(n)
        paths = []
        for s in range(args.files):
            p = os.path.join(tmp, f"song{s:02d}.wav")
            audio_io.write_wav(p, np.clip(np.roll(first, 7919 * s, axis=1).T, -0.99, 0.99), SR, "PCM_16")
            paths.append(p)
        log = logging.getLogger("probe.pitch")
        log.setLevel(logging.CRITICAL)

        def separator(model, out_dir, pitch_shift):
            cfg, sd, name, arch = model
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "model_name": name, "model_path": name + ".ckpt", "model_data": cfg.as_model_data(), "asx_state_dict": sd,
                      "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, out_dir), "normalization_threshold": 0.9,
                      "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False, "sample_rate": SR,
                      "use_soundfile": False, "asx_profile_file": True}
            return MDXCSeparator(common_config=common, arch_config=dict(arch, segment_size=256, override_model_segment_size=False, batch_size=1,
                                                                        pitch_shift=pitch_shift))

        def timed(call, after):
            walls = []
            for i in range(args.calls + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                if i:                                           # the first call warms workspaces, pinned staging and the page cache
                    walls.append(time.perf_counter() - t0)
                after(bool(i))
            return {"wall_ms_median": round(statistics.median(walls) * 1e3, 2), "wall_ms_spread": round((max(walls) - min(walls)) * 1e3, 2),
                    "wall_ms": [round(w * 1e3, 2) for w in walls]}

        out = {"what": f"MDXCSeparator on {args.seconds:g}-s PCM_16 WAVs on tmpfs -> 2 stem files each: separate(one file), separate_many({args.files} files)",
               "tree": args.label or os.path.abspath(args.tree), "rows": {}}
        for net in args.nets.split(","):
            model = make_model(net)
            for shift in (int(v) for v in args.shifts.split(",")):
                sep = separator(model, f"{net}_{shift}", shift)
                phases = {}

                def after(counted, sep=sep, phases=phases):
                    if counted:
                        for k, v in sep.file_timings.items():
                            phases[k] = phases.get(k, 0.0) + v
                    sep.clear_file_specific_paths()
                row = timed(lambda sep=sep: sep.separate(paths[0]), after)
                row["phases_ms"] = {k: round(v / args.calls * 1e3, 2) for k, v in phases.items()}
                row["decoded_on_device"] = "h2d_decode" in phases
                out["rows"][f"{net}, pitch_shift={shift}, one file"] = row
                if args.files > 1 and hasattr(sep, "separate_many"):
                    def many(sep=sep):
                        got = sep.separate_many(paths)
                        assert not sep.batch_errors and all(len(g) == 2 for g in got), sep.batch_errors
                    out["rows"][f"{net}, pitch_shift={shift}, separate_many({args.files} files)"] = timed(many, lambda counted: None)
                sep.clear_gpu_cache()
                for dm in sep._demixers.values():
                    dm.engine.close()
                del sep
                torch.cuda.empty_cache()
            del model
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
