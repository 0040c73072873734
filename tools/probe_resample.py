#!/usr/bin/env python3
"""What bringing a 4-minute stereo PCM16 file at 48 kHz or 96 kHz to 44.1 kHz costs with ``asx_input_resample = "device"``:

  kernel  asx_resample_rational_dev alone (device events over repeated launches, after a warm-up) next to its HBM floor: the bytes it must
          read and write over the bandwidth a device-to-device copy of the same bytes reaches in the same process; and asx_pcm_decode_dev
          of the file's data chunk, the step in front of it;
  file    ``MDXSeparator.separate(song.wav)`` on the HQ_3 geometry, file to files on tmpfs, for the 48 kHz file next to the same song at
          44.1 kHz (per-phase times from ``asx_profile_file``);
  host    the only alternative on an installation without librosa: scipy.signal.resample_poly(x, L, M, window=<the same taps>) on the host
          plus the upload of the float mix.

Every step runs in a fresh child process under a time limit of its own; the first one that fails ends the run.  One JSON object, also
written to --out.

    python tools/probe_resample.py [--seconds 240] [--out profiles/resample.json]
"""
import argparse
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
RATES = (48000, 96000)
STEPS = (("kernel", 300), ("file", 420), ("host", 420))      # (step, time limit in seconds)


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


def taps(rate):
    """The converter's filter, restated (csrc/resample_plan.h): (L, M, taps float64)."""
    from scipy.signal import kaiserord
    g = math.gcd(rate, SR)
    L, M = SR // g, rate // g
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
    out = {}

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps

    for rate in RATES:
        n_in = int(rate * args.seconds)
        n_out, L, M, T = eng.resample_rational_plan(rate, SR, n_in)
        pcm = torch.randint(-20000, 20000, (n_in, 2), dtype=torch.int16, device=dev)
        x = torch.empty((2, n_in), dtype=torch.float32, device=dev)
        y = torch.empty((2, n_out), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        decode_ms = timed(lambda: eng.pcm_decode_dev(pcm.data_ptr(), n_in, 2, "PCM_16", x.data_ptr(), stream=st, want_peak=False), 10)
        kernel_ms = timed(lambda: eng.resample_rational_dev(x.data_ptr(), 2, n_in, rate, SR, y.data_ptr(), n_out, stream=st), 20)
        # the floor: a copy that reads the input's bytes and writes the output's, i.e. (n_in + n_out) / 2 floats per channel each way
        nbytes = 4 * 2 * (n_in + n_out)
        half = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
        dst = torch.empty_like(half)
        copy_ms = timed(lambda: dst.copy_(half), 20)
        out[str(rate)] = {"n_in": n_in, "n_out": n_out, "L": L, "M": M, "taps_per_output": T,
                          "kernel_ms": round(kernel_ms, 4), "bytes_read_plus_written": nbytes,
                          "copy_same_bytes_ms": round(copy_ms, 4), "copy_gb_per_s": round(nbytes / copy_ms / 1e6, 1),
                          "kernel_over_floor": round(kernel_ms / copy_ms, 2),
                          "gflop_per_s": round(2.0 * 2 * n_out * T / kernel_ms / 1e6, 1),
                          "pcm_decode_ms": round(decode_ms, 4)}
    eng.close()
    return out


def step_file(args):
    import logging
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from workload import synth as O
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_probe_resample_", dir=base)
    try:
        wavs = {}
        for rate in (SR, 48000):
            wavs[rate] = os.path.join(tmp, f"song{rate}.wav")
            audio_io.write_wav(wavs[rate], np.ascontiguousarray(song(rate, args.seconds).T), rate, "PCM_16")
        d = O.NetDims()
        log = logging.getLogger("probe.resample")
        log.setLevel(logging.ERROR)
        common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                  "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": "UVR-MDX-NET-Inst_HQ_3", "model_path": None,
                  "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                 "primary_stem": "Instrumental"},
                  "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, "out"),
                  "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                  "sample_rate": SR, "use_soundfile": False, "asx_state_dict": O.make_convtdf_state(d, seed=0), "asx_net_config": A.NetConfig(),
                  "asx_profile_file": True, "asx_input_resample": "device"}
        arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
        sep = MDXSeparator(common, arch)

        def run(wav, calls):
            walls, phases = [], {}
            for _ in range(calls):
                t0 = time.perf_counter()
                sep.separate(wav)
                walls.append(time.perf_counter() - t0)
                for k, v in sep.file_timings.items():
                    phases[k] = phases.get(k, 0.0) + v
                sep.clear_gpu_cache()
                sep.clear_file_specific_paths()
            return {"wall_ms": round(sum(walls) / calls * 1e3, 2), "walls_ms": [round(w * 1e3, 2) for w in walls],
                    "phases_ms": {k: round(v / calls * 1e3, 2) for k, v in phases.items()}}

        out = {}
        for rate in (SR, 48000):
            run(wavs[rate], 1)                              # warm-up: workspaces, the table, pinned staging, page cache
        for rep in range(2):                                # alternate the two files
            for rate in (SR, 48000):
                out.setdefault(str(rate), []).append(run(wavs[rate], 2))
        sep.engine.close()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def step_host(args):
    import torch
    from scipy.signal import resample_poly
    dev = torch.device("cuda", 0)
    out = {}
    for rate in RATES:
        L, M, h = taps(rate)
        x = song(rate, args.seconds)
        t0 = time.perf_counter()
        y = resample_poly(x, L, M, axis=1, window=(h / L).astype(np.float32))   # (resample_poly scales a given filter by L itself)
        t1 = time.perf_counter()
        yd = torch.from_numpy(np.ascontiguousarray(y, np.float32)).to(dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        out[str(rate)] = {"resample_poly_ms": round((t1 - t0) * 1e3, 1), "upload_ms": round((t2 - t1) * 1e3, 2), "n_out": int(yd.shape[1]),
                          "threads": "one host thread (scipy's upfirdn)"}
        # the upload once more, warm
        t3 = time.perf_counter()
        torch.from_numpy(np.ascontiguousarray(y, np.float32)).to(dev)
        torch.cuda.synchronize(dev)
        out[str(rate)]["upload_warm_ms"] = round((time.perf_counter() - t3) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="run one step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"kernel": step_kernel, "file": step_file, "host": step_host}[args.step](args)))
        return 0
    res = {"what": f"{args.seconds:g} s stereo PCM16 at 48 / 96 kHz -> 44.1 kHz: asx_resample_rational_dev, the file-to-files wall of "
                   "MDXSeparator.separate, and scipy.signal.resample_poly with the same taps on the host", "seconds": args.seconds}
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--seconds", repr(args.seconds)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res[step] = {"error": f"time limit of {limit} s"}
            break
        if r.returncode != 0:
            res[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            break
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"probe_resample: step {step} done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if all("error" not in res.get(s, {"error": 1}) for s, _ in STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
