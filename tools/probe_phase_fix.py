#!/usr/bin/env python3
"""The phase fix (csrc/kernels_phasefix.h) on a 4-minute song: kernel time per stage beside asx_invert_stem_dev, and file to file.

    python tools/probe_phase_fix.py [--seconds 240] [--rounds 5] [--out FILE]

  kernels   asx_phase_fix_dev at hop 512 and hop 1024 on one 4-minute stereo stem pair in HBM, and asx_invert_stem_dev (hop 1024) on
            the same song: per stage (frames, fold) the engine's own device-event time per launch (asx_profile_launches), the median
            of ``--rounds`` calls after one warm-up; the time per frame workgroup pair and its ratio to the invert kernel's.
  files     PhaseFixSeparator on two resident MDXSeparator members (the HQ_3 geometry with narrow g = 8 nets and synthetic weights,
            so that the members' own time does not bury the edge): the device path against the host path (ASX_FILE_FASTPATH=0) in the
            same process on the same members and file, wall clock with the device drained, alternating order; outputs compared
            byte for byte.

One JSON line per figure."""
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
N_FFT = 2048


def emit(lines, **line):
    line = {"tool": "probe_phase_fix", **line}
    print(json.dumps(line), flush=True)
    lines.append(line)


def stage_ms(eng, call, rounds):
    """median device-event time of the "stft" (frames) and "ola" (fold) launches of ``call()`` and of its wall time, over ``rounds`` calls"""
    import torch
    call()
    torch.cuda.synchronize()
    frames, fold, wall = [], [], []
    for _ in range(rounds):
        eng.profile_enable(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        recs = eng.profile_launches()
        eng.profile_enable(False)
        frames.append(sum(ms for cls, ms, _, _ in recs if cls == "stft"))
        fold.append(sum(ms for cls, ms, _, _ in recs if cls == "ola"))
        assert len(recs) == 2, recs
    return statistics.median(frames), statistics.median(fold), statistics.median(wall)


def kernels(args, lines):
    import numpy as np
    import torch
    import audio_separator_amd as A
    from audio_separator_amd import phasefix
    from workload import synth as O
    n = int(SR * args.seconds)
    t = O.synth_mix(n, seed=0)
    s = (0.6 * np.roll(t, 5, axis=1) + 0.5 * O.synth_mix(n, seed=1)).astype(np.float32)
    eng = A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))
    dev = torch.device("cuda", eng.device)
    td, sd = torch.tensor(t, device=dev), torch.tensor(s, device=dev)
    out = torch.empty((2, n), dtype=torch.float32, device=dev)
    w = phasefix.bin_weights(SR)
    n_inv = 1024 * (n // 1024)
    inv_out = torch.empty((n_inv, 2), dtype=torch.float32, device=dev)
    f_inv, o_inv, w_inv = stage_ms(eng, lambda: eng.invert_stem_dev(td.data_ptr(), sd.data_ptr(), n, "planar", 1.0, inv_out.data_ptr(), n_inv), args.rounds)
    T_inv = 1 + n // 1024
    emit(lines, what="asx_invert_stem_dev", hop=1024, seconds=args.seconds, frames=T_inv, frame_ms=round(f_inv, 4), fold_ms=round(o_inv, 4),
         wall_ms=round(w_inv, 4), us_per_frame=round(1e3 * f_inv / T_inv, 4))
    for hop in (512, 1024):
        T = 1 + n // hop
        f, o, wall = stage_ms(eng, lambda: eng.phase_fix_dev((td.data_ptr(), "planar", n), (sd.data_ptr(), "planar", n), (out.data_ptr(), "planar"), w, hop),
                              args.rounds)
        emit(lines, what="asx_phase_fix_dev", hop=hop, seconds=args.seconds, frames=T, workspace_mb=round(2 * T * N_FFT * 4 / 1e6, 1),
             frame_ms=round(f, 4), fold_ms=round(o, 4), wall_ms=round(wall, 4), us_per_frame=round(1e3 * f / T, 4),
             per_frame_over_invert=round((f / T) / (f_inv / T_inv), 4), fold_over_invert=round(o / o_inv, 4))
    assert bool(torch.isfinite(out).all())
    eng.close()


def files(args, lines):
    import numpy as np
    import torch
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from workload import synth as O
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_phasefix_", dir=base)
    log = logging.getLogger("probe.phasefix")
    log.setLevel(logging.ERROR)
    saved = os.environ.get("ASX_FILE_FASTPATH")
    try:
        d = O.NetDims(g=8)
        members = []
        for k in range(2):
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": f"UVR-MDX-NET-narrow_{k}", "model_path": None,
                      "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                     "primary_stem": "Vocals"},
                      "output_format": "WAV", "output_bitrate": None, "output_dir": os.path.join(tmp, "out"),
                      "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                      "sample_rate": SR, "use_soundfile": False, "asx_state_dict": O.make_convtdf_state(d, seed=k), "asx_net_config": A.NetConfig(g=8)}
            arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
            members.append(MDXSeparator(common, arch))
        fixer = A.PhaseFixSeparator(members[0], members[1])
        path = os.path.join(tmp, "song.wav")
        audio_io.write_wav(path, np.ascontiguousarray(O.synth_mix(int(SR * args.seconds), seed=0).T), SR, "PCM_16")
        legs = {"device": ("1", os.path.join(tmp, "out_device")), "files": ("0", os.path.join(tmp, "out_files"))}

        def call(leg):
            os.environ["ASX_FILE_FASTPATH"], members[0].output_dir = legs[leg]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            names = fixer.separate(path)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if fixer.last_path_taken != leg:
                sys.exit(f"probe_phase_fix.py: the {leg} leg took the {fixer.last_path_taken} path")
            return [os.path.join(legs[leg][1], x) for x in names], ms

        outs = {leg: call(leg)[0] for leg in ("files", "device")}          # warm-up: workspaces, pinned staging, page cache
        same = len(outs["files"]) == len(outs["device"]) == 1 and filecmp.cmp(outs["files"][0], outs["device"][0], shallow=False)
        ms = {"files": [], "device": []}
        for r in range(max(3, args.rounds)):
            for leg in (("files", "device") if r % 2 == 0 else ("device", "files")):
                ms[leg].append(call(leg)[1])
        med = {leg: statistics.median(v) for leg, v in ms.items()}
        for leg in ("files", "device"):
            emit(lines, what="PhaseFixSeparator.separate", leg=leg, seconds=args.seconds, ms=[round(x, 2) for x in ms[leg]], median_ms=round(med[leg], 2),
                 spread=round((max(ms[leg]) - min(ms[leg])) / med[leg], 4))
        emit(lines, what="PhaseFixSeparator.separate", device_over_files=round(med["device"] / med["files"], 4), outputs_byte_identical=bool(same))
    finally:
        if saved is None:
            os.environ.pop("ASX_FILE_FASTPATH", None)
        else:
            os.environ["ASX_FILE_FASTPATH"] = saved
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("probe_phase_fix.py: no GPU (there is no CPU path to time)")
    lines = []
    kernels(args, lines)
    if not args.skip_files:
        files(args, lines)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
