#!/usr/bin/env python3
"""An ensemble of K resident models on one file: the device path of EnsembleSeparator against its file path.

    python tools/bench_ensemble.py [--members 3] [--workloads song,clips] [--algorithm avg_wave] [--rounds 3] [--out FILE]

K MDXSeparator members at the HQ_3 geometry with synthetic weights (workload/synth.py, one seed per member), kept resident.
Both legs run in the same process on the same members and the same PCM16 WAV files (tmpfs when there is one):

  files    EnsembleSeparator(via_files=True): every member's ``separate`` into a temporary directory (16-bit intermediate
           files), the files read back, ``Engine.ensemble`` on the host arrays, ``write_audio`` -- the reference's flow with the
           model reloads removed, and the nearest thing a checkout without ensemble.py can do.  THE BASELINE.
  device   EnsembleSeparator(): ``stems_dev`` -> asx_ensemble_slot_dev -> asx_ensemble_dev -> ``write_audio``; no intermediate file.

  song     one 4-minute song
  clips    8 clips of 20 s, one ``separate([...])`` call

One warm-up call per leg and workload, then ``--rounds`` rounds in alternating order (files, device, device, files, ...), each
call timed by wall clock with the device drained; per (workload, leg) every call, the median and the spread (max - min) / median,
and device / files per workload.  The outputs of the two legs are compared byte for byte once per workload."""
import argparse
import filecmp
import json
import logging
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
WORKLOADS = {"song": (1, 240.0, "one 4-minute song"), "clips": (8, 20.0, "8 clips x 20 s")}


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def run(args):
    import numpy as np
    import torch
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from workload import synth as O
    if not torch.cuda.is_available():
        sys.exit("bench_ensemble.py: no GPU (there is no CPU path to time)")
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_ensemble_", dir=base)
    log = logging.getLogger("bench.ensemble")
    log.setLevel(logging.ERROR)
    try:
        d = O.NetDims()
        members = []
        for k in range(args.members):
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": f"UVR-MDX-NET-synthetic_{k}", "model_path": None,
                      "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                     "primary_stem": "Instrumental"},
                      "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, "out"),
                      "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                      "sample_rate": SR, "use_soundfile": False, "asx_state_dict": O.make_convtdf_state(d, seed=k), "asx_net_config": A.NetConfig()}
            arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
            members.append(MDXSeparator(common, arch))
        names = [f"UVR-MDX-NET-synthetic_{k}.onnx" for k in range(args.members)]
        weights = [1.0 + 0.5 * k for k in range(args.members)] if args.algorithm.startswith("avg_") else None
        legs = {"files": A.EnsembleSeparator(members, args.algorithm, weights, model_filenames=names, via_files=True),
                "device": A.EnsembleSeparator(members, args.algorithm, weights, model_filenames=names)}
        for leg, ens in legs.items():
            ens.output_dir = os.path.join(tmp, "out_" + leg)
        lines = []
        for w in args.workloads.split(","):
            count, seconds, what = WORKLOADS[w]
            n = int(SR * seconds)
            first = O.synth_mix(n, seed=0)
            paths = []
            for s in range(count):
                path = os.path.join(tmp, f"{w}_{s}.wav")
                audio_io.write_wav(path, np.ascontiguousarray(np.roll(first, 7919 * s, axis=1).T), SR, "PCM_16")
                paths.append(path)

            def call(leg):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                files = legs[leg].separate(paths)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if legs[leg].last_path_taken != leg:
                    sys.exit(f"bench_ensemble.py: the {leg} leg took the {legs[leg].last_path_taken} path")
                return files, ms

            outs = {leg: call(leg)[0] for leg in ("files", "device")}          # warm-up: workspaces, pinned staging, page cache
            same = len(outs["files"]) == len(outs["device"]) and all(filecmp.cmp(a, b, shallow=False)
                                                                     for a, b in zip(outs["files"], outs["device"]))
            ms = {"files": [], "device": []}
            for r in range(args.rounds):
                for leg in (("files", "device") if r % 2 == 0 else ("device", "files")):
                    ms[leg].append(call(leg)[1])
            med = {leg: statistics.median(v) for leg, v in ms.items()}
            for leg in ("files", "device"):
                line = {"tool": "bench_ensemble", "workload": w, "what": what, "leg": leg, "baseline": leg == "files", "members": args.members,
                        "algorithm": args.algorithm, "inputs": count, "seconds_per_input": seconds, "rounds": args.rounds,
                        "outputs": len(outs[leg]), "ms": [round(x, 2) for x in ms[leg]], "median_ms": round(med[leg], 2),
                        "spread": round(spread(ms[leg]), 5), "audio_s_per_wall_s": round(count * seconds / (med[leg] * 1e-3), 2)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            line = {"tool": "bench_ensemble", "workload": w, "device_over_files": round(med["device"] / med["files"], 4),
                    "outputs_byte_identical": bool(same)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            for p in paths:
                os.remove(p)
        if args.out:
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--workloads", default="song,clips")
    ap.add_argument("--algorithm", default="avg_wave")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        sys.exit("bench_ensemble.py: at least 3 rounds")
    if not 2 <= args.members <= 8:
        sys.exit("bench_ensemble.py: 2 .. 8 members")
    run(args)


if __name__ == "__main__":
    main()
