#!/usr/bin/env python3
"""What ``EnsembleSeparator(intermediate="writer")`` and ``output_rate="input"`` cost and save on studio material: a 4-minute 24-bit
48 kHz WAV on tmpfs through two resident MDX members at the HQ_3 geometry (synthetic weights, ``asx_input_resample="device"``),
file to files, wall clock with the device drained.

  default       members without soundfile, ``EnsembleSeparator()``: the device path with the 16-bit intermediates -- on BOTH trees; the
                only bar of this probe is that the two agree within the run's own spread
  files         members with ``use_soundfile=True``, ``EnsembleSeparator()``: the soundfile writer sends the ensemble through
                intermediate files -- what the parent commit does with such members, on both trees
  writer        the same members, ``intermediate="writer"``: the device path with PCM_24 slot images (this tree only)
  writer_input  ... plus ``output_rate="input"``: the result converted back to 48 kHz inside the writer (this tree only)

With --parent TREE (a checkout of the parent commit with its library built) children of the two trees alternate; every child is a fresh
process under a time limit of its own that runs its configurations in rotation, one warm-up call each, then --calls measured calls
(the median is reported).  The first child that fails ends the run.  One JSON object, also written to --out.

    python tools/probe_ensemble_writer.py [--seconds 240] [--parent TREE] [--out profiles/ensemble_writer.json]
"""
import argparse
import json
import logging
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SR = 44100
FILE_RATE = 48000
LIMIT = 900                                                 # time limit of a child, seconds
CONFIGS = {"default": (False, {}, "device"), "files": (True, {}, "files"), "writer": (True, {"intermediate": "writer"}, "device"),
           "writer_input": (True, {"intermediate": "writer", "output_rate": "input"}, "device")}   # (soundfile members?, arguments, path)


def song(rate, seconds):
    """Deterministic stereo programme material at ``rate``: a few partials per channel under a slow envelope, peak about 0.8."""
    n = int(rate * seconds)
    t = np.arange(n, dtype=np.float64) / rate
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 0.37 * t)
    chans = []
    for c in range(2):
        x = np.zeros(n)
        for k, f in enumerate((110.0, 440.0 * (1 + 0.01 * c), 1760.0, 7040.0, 15000.0)):
            x += np.sin(2 * np.pi * f * t + 0.7 * k + c) / (k + 1)
        chans.append(0.8 * env * x / 2.3)
    return np.asarray(chans, np.float32)


def step(args):
    """One child: the configurations of --configs on the package imported from --tree."""
    import torch
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from workload import synth as O
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_probe_ensemble_writer_", dir=base)
    log = logging.getLogger("probe.ensemble_writer")
    log.setLevel(logging.ERROR)
    try:
        wav = os.path.join(tmp, "studio.wav")
        audio_io.write_wav(wav, np.ascontiguousarray(song(FILE_RATE, args.seconds).T), FILE_RATE, "PCM_24")
        d = O.NetDims()
        names = [f"UVR-MDX-NET-synthetic_{k}.onnx" for k in range(2)]

        def members(soundfile):
            out = []
            for k in range(2):
                common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                          "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": f"UVR-MDX-NET-synthetic_{k}", "model_path": None,
                          "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                         "primary_stem": "Instrumental"},
                          "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, "out"),
                          "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                          "sample_rate": SR, "use_soundfile": soundfile, "asx_state_dict": O.make_convtdf_state(d, seed=k),
                          "asx_net_config": A.NetConfig(), "asx_input_resample": "device", "asx_output_encoder": "device"}
                arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
                out.append(MDXSeparator(common, arch))
            return out

        configs = args.configs.split(",")
        sets = {sf: members(sf) for sf in sorted({CONFIGS[c][0] for c in configs})}
        legs = {}
        for c in configs:
            soundfile, kw, _ = CONFIGS[c]
            legs[c] = A.EnsembleSeparator(sets[soundfile], "avg_wave", [1.0, 1.5], model_filenames=names, **kw)
            legs[c].output_dir = os.path.join(tmp, "out_" + c)
        walls, outputs = {c: [] for c in configs}, {}
        for rep in range(args.calls + 1):                   # rep 0 is the warm-up: workspaces, the tables, pinned staging, page cache
            for c in (configs if rep % 2 == 0 else configs[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                files = legs[c].separate(wav)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                if legs[c].last_path_taken != CONFIGS[c][2]:
                    raise SystemExit(f"probe_ensemble_writer.py: {c} took the {legs[c].last_path_taken} path")
                if rep:
                    walls[c].append(wall)
                outputs[c] = files
        out = {"tree": "parent commit" if os.path.abspath(args.tree) != ROOT else "this commit"}
        for c in configs:
            info = [audio_io.wav_info(f) for f in outputs[c]]
            out[c] = {"median_wall_ms": round(statistics.median(walls[c]) * 1e3, 2), "walls_ms": [round(w * 1e3, 2) for w in walls[c]],
                      "spread": round((max(walls[c]) - min(walls[c])) / statistics.median(walls[c]), 4),
                      "outputs": [(i["samplerate"], i["frames"], i["subtype"]) for i in info]}
        if "files" in outputs and "writer" in outputs:
            out["writer_equals_files_byte_for_byte"] = all(open(a, "rb").read() == open(b, "rb").read()
                                                           for a, b in zip(outputs["writer"], outputs["files"]))
        for group in sets.values():
            for m in group:
                m.engine.close()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def child(args, tree, configs):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--seconds", repr(args.seconds), "--tree", tree, "--configs", configs,
           "--calls", str(args.calls)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        return {"error": f"time limit of {LIMIT} s"}
    if r.returncode != 0:
        return {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--calls", type=int, default=5, help="measured separate() calls per child and configuration (the median is reported)")
    ap.add_argument("--rounds", type=int, default=2, help="children per tree, alternating")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its children alternate with this tree's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help="run the configurations in this process (what the driver starts)")
    ap.add_argument("--tree", default=ROOT, help="with --step: the tree whose package is imported")
    ap.add_argument("--configs", default="default,files,writer,writer_input")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, os.path.abspath(args.tree))
        print(json.dumps(step(args)))
        return 0
    res = {"what": f"{args.seconds:g} s 24-bit {FILE_RATE} Hz WAV on tmpfs, two MDX members at the HQ_3 geometry, avg_wave: file-to-files wall of "
                   "EnsembleSeparator.separate per configuration, medians per child", "seconds": args.seconds, "children": []}
    ok = True
    for _ in range(args.rounds):
        for tree, configs in (((args.parent, "default,files"),) if args.parent else ()) + ((ROOT, args.configs),):
            res["children"].append(child(args, tree, configs))
            failed = "error" in res["children"][-1]
            print(f"probe_ensemble_writer: child of {tree} {'FAILED' if failed else 'done'}", file=sys.stderr, flush=True)
            if failed:                                      # nothing more is started on the device after a failure
                ok = False
                break
        if not ok:
            break
    if ok:
        summary = {}
        for c in CONFIGS:
            for tree in ("parent commit", "this commit"):
                meds = [ch[c]["median_wall_ms"] for ch in res["children"] if ch["tree"] == tree and c in ch]
                if meds:
                    summary.setdefault(c, {})[tree] = {"median_of_children_ms": round(statistics.median(meds), 2), "children_ms": meds}
        res["summary"] = summary
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
