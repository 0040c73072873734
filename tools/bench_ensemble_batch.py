#!/usr/bin/env python3
"""A batch of files through an ensemble of K resident models: ``EnsembleSeparator.separate_many(paths)`` -- every member pools the
chunks of all files per net pass, one pooled device call combines the stems of all (file, stem group) pairs -- against the loop.

    python tools/bench_ensemble_batch.py [--members 3] [--workloads clips64,songs8] [--legs loop,batch] [--algorithm avg_wave]
                                         [--rounds 3] [--out FILE]

K MDXSeparator members at the HQ_3 geometry with synthetic weights (workload/synth.py, one seed per member), kept resident -- the
members of tools/bench_ensemble.py.  Both legs run in the same process on the same members and the same PCM16 WAV files (tmpfs
when there is one):

  loop     ``separate(paths)``: the device path file by file (``stems_dev`` -> asx_ensemble_slot_dev -> asx_ensemble_dev ->
           ``write_audio``).  THE BASELINE; ``--legs loop`` also runs on a checkout without ``separate_many``.
  batch    ``separate_many(paths)``.

  clips64  64 clips of 20 s
  songs8   8 songs of 4 minutes

One warm-up call per leg and workload, then ``--rounds`` rounds in alternating order (loop, batch, batch, loop, ...), each call
timed by wall clock with the device drained; per (workload, leg) every call, the median and the spread (max - min) / median, and
batch / loop per workload.  The outputs of the two legs are compared byte for byte once per workload."""
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
WORKLOADS = {"clips64": (64, 20.0, "64 clips x 20 s"), "songs8": (8, 240.0, "8 songs x 4 min"), "clips4": (4, 5.0, "4 clips x 5 s (a quick look)")}


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
        sys.exit("bench_ensemble_batch.py: no GPU (there is no CPU path to time)")
    leg_names = args.legs.split(",")
    if "batch" in leg_names and not hasattr(A.EnsembleSeparator, "separate_many"):
        sys.exit("bench_ensemble_batch.py: this checkout has no EnsembleSeparator.separate_many (run --legs loop)")
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_ensemble_batch_", dir=base)
    log = logging.getLogger("bench.ensemble_batch")
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
        legs = {leg: A.EnsembleSeparator(members, args.algorithm, weights, model_filenames=names) for leg in leg_names}
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
                ens = legs[leg]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if leg == "loop":
                    files = ens.separate(paths)
                    taken = [ens.last_path_taken]
                else:
                    files = [f for fs in ens.separate_many(paths) for f in fs]
                    taken = ens.last_paths_taken
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if any(t != "device" for t in taken):
                    sys.exit(f"bench_ensemble_batch.py: the {leg} leg left the device path ({taken})")
                return files, ms

            outs = {leg: call(leg)[0] for leg in leg_names}                    # warm-up: workspaces, pinned staging, page cache
            same = None
            if len(leg_names) == 2:
                a, b = (outs[leg] for leg in leg_names)
                same = len(a) == len(b) == 2 * count and all(os.path.basename(x) == os.path.basename(y) and filecmp.cmp(x, y, shallow=False)
                                                             for x, y in zip(a, b))
            ms = {leg: [] for leg in leg_names}
            for r in range(args.rounds):
                for leg in (leg_names if r % 2 == 0 else leg_names[::-1]):
                    ms[leg].append(call(leg)[1])
            med = {leg: statistics.median(v) for leg, v in ms.items()}
            for leg in leg_names:
                line = {"tool": "bench_ensemble_batch", "workload": w, "what": what, "leg": leg, "baseline": leg == "loop", "members": args.members,
                        "algorithm": args.algorithm, "inputs": count, "seconds_per_input": seconds, "rounds": args.rounds,
                        "outputs": len(outs[leg]), "ms": [round(x, 2) for x in ms[leg]], "median_ms": round(med[leg], 2),
                        "spread": round(spread(ms[leg]), 5), "audio_s_per_wall_s": round(count * seconds / (med[leg] * 1e-3), 2)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            if len(leg_names) == 2:
                line = {"tool": "bench_ensemble_batch", "workload": w, "batch_over_loop": round(med["batch"] / med["loop"], 4),
                        "outputs_byte_identical": bool(same)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            for p in paths:
                os.remove(p)
            for leg in leg_names:
                shutil.rmtree(legs[leg].output_dir, ignore_errors=True)
        if args.out:
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--workloads", default="clips64,songs8")
    ap.add_argument("--legs", default="loop,batch")
    ap.add_argument("--algorithm", default="avg_wave")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        sys.exit("bench_ensemble_batch.py: at least 3 rounds")
    if not 2 <= args.members <= 8:
        sys.exit("bench_ensemble_batch.py: 2 .. 8 members")
    if args.legs not in ("loop,batch", "batch,loop", "loop", "batch"):
        sys.exit("bench_ensemble_batch.py: --legs is loop, batch or both")
    if any(w not in WORKLOADS for w in args.workloads.split(",")):
        sys.exit(f"bench_ensemble_batch.py: workloads are {sorted(WORKLOADS)}")
    run(args)


if __name__ == "__main__":
    main()
