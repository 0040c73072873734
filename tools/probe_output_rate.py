#!/usr/bin/env python3
"""What writing the stems of a 4-minute song back at the input file's rate costs with ``asx_output_rate = "input"``:

  kernel  asx_resample_rational_stem_dev alone (device events over 20 launches, after a warm-up) for the stems of the song at 44.1 kHz
          -- MDX rows [N, 2], and the four Demucs stems planar [4, 2, N] in one launch -- to 48 kHz and to 96 kHz; beside it, as the
          yardstick, asx_resample_rational_dev 48 kHz -> 44.1 kHz on the same song (the input side of the same file);
          and the complement form of the same launch, asx_resample_rational_complement_dev (``asx_complement_rate = "input"``), on the
          MDX rows stem against a file-rate mix [2, F]: y and c stored, and c alone;
  file    ``MDXSeparator.separate(song.wav)`` on the HQ_3 geometry, file to files on tmpfs, PCM_16 in at --rate (48 kHz): medians of 5 per
          child process with ``asx_output_rate`` off and on, and with ``asx_complement_rate = "input"`` on top, alternating; with --parent
          TREE (a checkout of the parent commit with its library built) that tree's run at --parent-knob ("off", or "on": asx_output_rate =
          "input", the path the complement knob must not slow down) alternates with this one's, child by child;
  host    the alternative on the host: scipy.signal.resample_poly(stem, L, M, window=<the same taps>) per stereo stem -- ONE host thread.

Every step runs in a fresh child process under a time limit of its own; the first one that fails ends the run.  One JSON object, also
written to --out.

    python tools/probe_output_rate.py [--seconds 240] [--parent TREE] [--out profiles/output_rate.json]
"""
import argparse
import json
import math
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
RATES = (48000, 96000)
LIMITS = {"kernel": 300, "file": 420, "host": 420}      # time limit of a child, seconds


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


def taps(sr_in, sr_out):
    """The converter's filter, restated (csrc/resample_plan.h): (L, M, taps float64)."""
    from scipy.signal import kaiserord
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    G = max(L, M)
    fpass, fstop = 0.913 / G, 1.0 / G
    N, beta = kaiserord(125.0, fstop - fpass)
    half = -(-(N - 1) // (2 * L)) * L
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = 0.5 * (fpass + fstop)
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
    return L, M, h * (L / h.sum())


def step_kernel(args):
    import torch
    import audio_separator_amd as A
    eng = A.Engine(A.MDXConfig())
    dev = torch.device("cuda", eng.device)
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {}

    def timed(fn, reps=20):
        fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps

    n = int(SR * args.seconds)
    mix = torch.from_numpy(song(SR, args.seconds)).to(dev)                      # [2, N]
    rows = mix.T.contiguous()                                                   # the MDX stem layout [N, 2]
    four = torch.stack([mix * s for s in (1.0, 0.7, 0.5, 0.3)]).contiguous()    # the Demucs layout [4, 2, N]
    for rate in RATES:
        F = int(rate * args.seconds)
        _, L, M, T = eng.resample_rational_plan(SR, rate, n)
        y = torch.empty((8, F), dtype=torch.float32, device=dev)
        r = {"n_in": n, "n_out": F, "L": L, "M": M, "taps_per_output": T}
        for name, x, layout, ch in (("mdx_rows_2ch", rows, "rows", 2), ("planar_2ch", mix, "planar", 2), ("demucs_planar_8ch", four, "planar", 8)):
            ms = timed(lambda: eng.resample_rational_stem_dev(x.data_ptr(), layout, ch, n, SR, rate, y.data_ptr(), F, stream=st))
            r[name] = {"kernel_ms": round(ms, 4), "gflop_per_s": round(2.0 * ch * F * T / ms / 1e6, 1),
                       "gb_per_s_read_plus_written": round(4.0 * ch * (n + F) / ms / 1e6, 1)}
        if hasattr(eng, "resample_rational_complement_dev"):
            file_mix = torch.from_numpy(song(rate, args.seconds)).to(dev)[:, :F].contiguous()      # the file's own mix [2, F]
            c = torch.empty((2, F), dtype=torch.float32, device=dev)
            for name, y_ptr, stores in (("complement_rows_2ch", y.data_ptr(), 2), ("complement_rows_2ch_c_only", 0, 1)):
                ms = timed(lambda: eng.resample_rational_complement_dev(rows.data_ptr(), "rows", 2, n, SR, rate, file_mix.data_ptr(), F, 0.95,
                                                                        1.022, y_ptr, c.data_ptr(), F, stream=st))
                r[name] = {"kernel_ms": round(ms, 4), "gflop_per_s": round(2.0 * 2 * F * T / ms / 1e6, 1),
                           "gb_per_s_read_plus_written": round(4.0 * 2 * (n + F * (1 + stores)) / ms / 1e6, 1)}
        out[f"{SR}->{rate}"] = r
    # the yardstick: the input side of the same 48 kHz file
    n48 = int(48000 * args.seconds)
    n_out, L, M, T = eng.resample_rational_plan(48000, SR, n48)
    x48 = torch.from_numpy(song(48000, args.seconds)).to(dev)
    y = torch.empty((2, n_out), dtype=torch.float32, device=dev)
    ms = timed(lambda: eng.resample_rational_dev(x48.data_ptr(), 2, n48, 48000, SR, y.data_ptr(), n_out, stream=st))
    out[f"48000->{SR} (asx_resample_rational_dev)"] = {"n_in": n48, "n_out": n_out, "L": L, "M": M, "taps_per_output": T, "kernel_ms": round(ms, 4),
                                                      "gflop_per_s": round(2.0 * 2 * n_out * T / ms / 1e6, 1)}
    eng.close()
    return out


def step_file(args):
    """One child: the knob-off run (and, for this tree, the knob-on run, alternating) of the package imported from --tree."""
    import logging
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from workload import synth as O
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_probe_output_rate_", dir=base)
    try:
        wav = os.path.join(tmp, f"song{args.rate}.wav")
        audio_io.write_wav(wav, np.ascontiguousarray(song(args.rate, args.seconds).T), args.rate, "PCM_16")
        d = O.NetDims()
        log = logging.getLogger("probe.output_rate")
        log.setLevel(logging.ERROR)
        common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                  "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": "UVR-MDX-NET-Inst_HQ_3", "model_path": None,
                  "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                 "primary_stem": "Instrumental"},
                  "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, "out"),
                  "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                  "sample_rate": SR, "use_soundfile": False, "asx_state_dict": O.make_convtdf_state(d, seed=0), "asx_net_config": A.NetConfig(),
                  "asx_profile_file": bool(args.phases), "asx_input_resample": "device"}
        arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
        knobs = {"both": ["off", "on"], "all": ["off", "on", "complement"]}.get(args.knob, [args.knob])
        over = {"off": {}, "on": {"asx_output_rate": "input"}, "complement": {"asx_output_rate": "input", "asx_complement_rate": "input"}}
        seps = {k: MDXSeparator(dict(common, **over[k]), arch) for k in knobs}
        walls, phases = {k: [] for k in knobs}, {k: {} for k in knobs}
        for rep in range(args.calls + 1):                   # rep 0 is the warm-up: workspaces, the tables, pinned staging, page cache
            for k in knobs:
                sep = seps[k]
                t0 = time.perf_counter()
                names = sep.separate(wav)
                wall = time.perf_counter() - t0
                if rep:
                    walls[k].append(wall)
                    for p, v in sep.file_timings.items():
                        phases[k].setdefault(p, []).append(v)
                sep.clear_gpu_cache()
                sep.clear_file_specific_paths()
        out = {"tree": "parent commit" if os.path.abspath(args.tree) != ROOT else "this commit", "rate": args.rate}
        for k in knobs:
            info = [audio_io.wav_info(os.path.join(common["output_dir"], n)) for n in names] if k == knobs[-1] else None
            out[k] = {"median_wall_ms": round(statistics.median(walls[k]) * 1e3, 2), "walls_ms": [round(w * 1e3, 2) for w in walls[k]],
                      "median_phases_ms": {p: round(statistics.median(v) * 1e3, 3) for p, v in phases[k].items()}}
            if info:
                out[k]["last_outputs"] = [(i["samplerate"], i["frames"]) for i in info]
        for sep in seps.values():
            sep.engine.close()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def step_host(args):
    from scipy.signal import resample_poly
    out = {}
    x = song(SR, args.seconds)
    for rate in RATES:
        L, M, h = taps(SR, rate)
        t0 = time.perf_counter()
        y = resample_poly(x, L, M, axis=1, window=(h / L).astype(np.float32))   # (resample_poly scales a given filter by L itself)
        out[f"{SR}->{rate}"] = {"resample_poly_ms_per_stereo_stem": round((time.perf_counter() - t0) * 1e3, 1), "n_out": int(y.shape[1]),
                                "threads": "one host thread (scipy's upfirdn)"}
    return out


def child(step, args, tree, knob="both", limit=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--seconds", repr(args.seconds), "--tree", tree, "--knob", knob,
           "--calls", str(args.calls), "--rate", str(args.rate)] + (["--phases"] if args.phases else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit or LIMITS[step])
    except subprocess.TimeoutExpired:
        return {"error": f"time limit of {limit or LIMITS[step]} s"}
    if r.returncode != 0:
        return {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--calls", type=int, default=5, help="measured separate() calls per child and knob (the median is reported)")
    ap.add_argument("--rounds", type=int, default=2, help="file step: children per tree, alternating")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: its knob-off run alternates with this tree's")
    ap.add_argument("--phases", action="store_true", help="file step: per-phase times (asx_profile_file drains the device per phase)")
    ap.add_argument("--steps", default="kernel,file,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(LIMITS), default=None, help="run one step in this process (what the driver starts)")
    ap.add_argument("--tree", default=ROOT, help="with --step: the tree whose package is imported")
    ap.add_argument("--knob", choices=["off", "on", "complement", "both", "all"], default="all")
    ap.add_argument("--parent-knob", choices=["off", "on"], default="off", help="what the parent tree's children run")
    ap.add_argument("--rate", type=int, default=48000, help="file step: the input file's sample rate")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, os.path.abspath(args.tree))
        print(json.dumps({"kernel": step_kernel, "file": step_file, "host": step_host}[args.step](args)))
        return 0
    res = {"what": f"{args.seconds:g} s of stereo stems at 44.1 kHz -> 48 / 96 kHz: asx_resample_rational_stem_dev, the file-to-files wall of "
                   f"its complement form, the file-to-files wall of MDXSeparator.separate on a {args.rate} Hz PCM_16 file with asx_output_rate off / "
                   "on / on with asx_complement_rate = 'input', and scipy.signal.resample_poly with the same taps on one host thread",
           "seconds": args.seconds}
    ok = True
    for step in args.steps.split(","):
        if step != "file":
            res[step] = child(step, args, ROOT)
        else:
            res[step] = []
            for _ in range(args.rounds):
                for tree, knob in (((args.parent, args.parent_knob),) if args.parent else ()) + ((ROOT, args.knob),):
                    res[step].append(child("file", args, tree, knob))
                    if "error" in res[step][-1]:
                        break
                if res[step] and "error" in res[step][-1]:
                    break
        failed = "error" in (res[step][-1] if isinstance(res[step], list) else res[step])
        print(f"probe_output_rate: step {step} {'FAILED' if failed else 'done'}", file=sys.stderr, flush=True)
        if failed:                                          # nothing more is started on the device after a failure
            ok = False
            break
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
