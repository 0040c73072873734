#!/usr/bin/env python3
"""What ``workflow.ChainSeparator`` costs and saves against the literal flow it reproduces: a 4-minute PCM_16 44.1 kHz WAV on tmpfs, the
MDX geometry of the headline (HQ_3, synthetic weights) at both stages, the second stage on the first one's Instrumental stem, file to
files, wall clock with the device drained.

  wav     ``separate`` with WAV stems:  literal = first.separate(path); then.separate(<the stem's file>)   chain = ChainSeparator.separate
  flac    the same with FLAC stems (the device encoder; the literal flow's second stage decodes the FLAC stem on the device)
  many8   eight copies of the file:     literal = first.separate_many(paths); then.separate_many(stem files)   chain = separate_many
  mixdown the kernel alone: one 4-minute "Instrumental + Vocals" mix-down (two rows stems -> planar), device events

The literal flow and the chain alternate call by call in ONE process on the same two resident plugins; one warm-up call each, then
--calls measured calls, medians reported.  The probe checks that the chain took the device path and that its files equal the literal
flow's byte for byte.  One JSON object, also written to --out.

    python tools/probe_chain.py [--seconds 240] [--calls 5] [--out profiles/chain_probe.json]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100


def song(rate, seconds):
    """Deterministic stereo programme material: a few partials per channel under a slow envelope, peak about 0.8."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--calls", type=int, default=5, help="measured calls per leg (the median is reported)")
    ap.add_argument("--files", type=int, default=8, help="files of the separate_many leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from audio_separator_amd.workflow import ChainSeparator
    from workload import synth as O

    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="asx_probe_chain_", dir=base)
    log = logging.getLogger("probe.chain")
    log.setLevel(logging.ERROR)
    res = {"what": f"{args.seconds:g} s PCM_16 {SR} Hz WAV on tmpfs, MDX HQ_3 geometry at both stages, the second on the first's Instrumental stem: "
                   "file-to-files wall of the literal flow and of ChainSeparator, alternating in one process", "seconds": args.seconds,
           "calls": args.calls}
    try:
        paths = []
        x = np.ascontiguousarray(song(SR, args.seconds).T)
        for i in range(args.files):
            paths.append(os.path.join(tmp, f"song{i}.wav"))
            audio_io.write_wav(paths[-1], x, SR, "PCM_16")
        d = O.NetDims()

        def stage(k, fmt):
            common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
                      "onnx_execution_provider": ["ROCMExecutionProvider"], "model_name": f"UVR-MDX-NET-synthetic_{k}", "model_path": None,
                      "model_data": {"compensate": 1.022, "mdx_dim_f_set": 3072, "mdx_dim_t_set": 8, "mdx_n_fft_scale_set": 6144,
                                     "primary_stem": "Vocals"},
                      "output_format": fmt, "output_bitrate": None, "output_dir": os.path.join(tmp, "out"),
                      "normalization_threshold": 0.9, "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False,
                      "sample_rate": SR, "use_soundfile": False, "asx_state_dict": O.make_convtdf_state(d, seed=k),
                      "asx_net_config": A.NetConfig()}
            arch = {"hop_length": 1024, "segment_size": 256, "overlap": 0.25, "batch_size": 1, "enable_denoise": False}
            return MDXSeparator(common, arch)

        def timed(call):
            for p in (first, then):                          # what the orchestrator does between files
                p.clear_file_specific_paths()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        def read_all(out_dir, names):
            return [open(os.path.join(out_dir, n), "rb").read() for n in names]

        first = then = None
        for leg, fmt, many in (("wav", "WAV", False), ("flac", "FLAC", False), ("many8", "WAV", True)):
            if first is None or first.output_format != fmt:
                for p in (first, then):
                    if p is not None:
                        p.engine.close()
                first, then = stage(0, fmt), stage(1, fmt)
            chain = ChainSeparator(first, then, "Instrumental")
            lit_dir, chain_dir = os.path.join(tmp, f"lit_{leg}"), os.path.join(tmp, f"chain_{leg}")

            def literal():
                first.output_dir = then.output_dir = lit_dir
                if many:
                    a = first.separate_many(paths)
                    b = then.separate_many([os.path.join(lit_dir, names[0]) for names in a])      # (the secondary stem comes first)
                    return [x + y for x, y in zip(a, b)]
                a = first.separate(paths[0])
                return a + then.separate(os.path.join(lit_dir, first.get_stem_output_path("Instrumental", None)))

            def chained():
                first.output_dir = then.output_dir = chain_dir
                return chain.separate_many(paths) if many else chain.separate(paths[0])

            walls = {"literal": [], "chain": []}
            names = {}
            for rep in range(args.calls + 1):               # rep 0 is the warm-up: workspaces, tables, pinned staging, page cache
                order = (("literal", literal), ("chain", chained)) if rep % 2 == 0 else (("chain", chained), ("literal", literal))
                for which, call in order:
                    wall, out = timed(call)
                    names[which] = out
                    if rep:
                        walls[which].append(wall)
                if chain.last_path_taken != "device" or (many and set(chain.last_paths_taken) != {"device"}):
                    raise SystemExit(f"probe_chain.py: {leg}: the chain took the {chain.last_path_taken} path")
            flat = (lambda v: [n for names_of in v for n in names_of]) if many else (lambda v: v)
            same = flat(names["literal"]) == flat(names["chain"]) and \
                read_all(lit_dir, flat(names["literal"])) == read_all(chain_dir, flat(names["chain"]))
            med = {k: statistics.median(v) for k, v in walls.items()}
            res[leg] = {"literal_median_ms": round(med["literal"] * 1e3, 2), "chain_median_ms": round(med["chain"] * 1e3, 2),
                        "chain_over_literal": round(med["chain"] / med["literal"], 4),
                        "literal_ms": [round(w * 1e3, 2) for w in walls["literal"]], "chain_ms": [round(w * 1e3, 2) for w in walls["chain"]],
                        "files_equal_byte_for_byte": bool(same), "handoff_gain": chain.last_handoff_gain}
            print(f"probe_chain: {leg} done", file=sys.stderr, flush=True)
            if not same:
                raise SystemExit(f"probe_chain.py: {leg}: the chain's files differ from the literal flow's")

        # the kernel alone: two rows stems of the song's length -> one planar mix-down
        n = x.shape[0]
        eng = then.engine
        a = torch.from_numpy(x).cuda()
        b = torch.from_numpy(np.ascontiguousarray(x[::-1])).cuda()
        out = torch.empty((2, n), dtype=torch.float32, device="cuda")
        job = [([(a.data_ptr(), "rows", n, 1.0), (b.data_ptr(), "rows", n, 1.0 / 0.93)], out.data_ptr(), "planar", n)]
        st = torch.cuda.current_stream().cuda_stream
        times = []
        for rep in range(args.calls + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.mixdown_batch_dev(job, stream=st)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        res["mixdown"] = {"frames": n, "sources": 2, "median_ms": round(ms, 4), "times_ms": [round(t, 4) for t in times],
                          "bytes": 24 * n, "TB_per_s": round(24 * n / (ms * 1e-3) / 1e12, 3)}
        for p in (first, then):
            p.engine.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
