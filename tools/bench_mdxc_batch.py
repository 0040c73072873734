#!/usr/bin/env python3
"""A batch of files through the MDXC plugin: ``MDXCSeparator.separate_many(paths)`` -- the chunks of all files pooled per net
pass -- against the loop of ``separate(path)`` over the same files.

    python tools/bench_mdxc_batch.py [--nets rof,mdx23c] [--workloads a,b] [--legs loop,pool] [--reps 5] [--tag NAME] [--out FILE]

Nets, synthetic weights, as tools/bench_siblings.py builds them: ``rof`` = the BS-Roformer ep_317 layout (8-s chunks, step = chunk,
16 chunks per net pass), ``mdx23c`` = the MDX23C layout (overlap 2, 8 chunks per net pass).  Inputs are 16-bit stereo WAV files at
44.1 kHz in a temporary directory, so both legs take the device-resident file path: read, decode, normalise, demix, write.  Before
anything is timed the two legs run once each into their own directories and every output file is compared byte for byte (that
pass is also the warm-up).  Then ``reps`` passes per leg, wall clock around the whole call with the device drained; one JSON line
per (net, workload, leg) with every pass, the median, the spread (max - min) / median and the net passes of one call.

  a   64 clips x 20 s
  b   8 songs x 4 min

The ``loop`` leg needs nothing this tool's commit added, so the same file run from a checkout of an earlier commit gives that
commit's baseline (no byte comparison there); ``--merge`` folds the lines of several runs into one record:

    python tools/bench_mdxc_batch.py --merge run1.jsonl run2.jsonl ... --out profiles/NAME_mdxc_batch_pool.json
"""
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
WORKLOADS = {"a": (64, 20.0, "64 clips x 20 s"), "b": (8, 240.0, "8 songs x 4 min")}
NETS = {"rof": "BS-Roformer ep_317 layout, overlap 8 (step = chunk), 16 chunks per pass",
        "mdx23c": "MDX23C layout, overlap 2, 8 chunks per pass"}


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def make_model(net):
    """(config, synthetic state dict, model name, arch options) of a net"""
    if net == "rof":
        from oracle import roformer_oracle as R
        cfg = R.RoformerConfig(freqs_per_bands=R.DEFAULT_FREQS_PER_BANDS)
        return cfg, R.make_roformer_state(cfg, 0), "bs_roformer_ep_317_layout", {"overlap": 8, "asx_max_batch": 16}
    from oracle import mdxc_oracle as M
    cfg = M.V3Config()
    return cfg, M.make_v3_state(cfg, 0), "mdx23c_layout", {"overlap": 2, "asx_max_batch": 8}


def make_separator(model, out_dir):
    from audio_separator_amd.architectures.mdxc_separator import MDXCSeparator
    cfg, sd, name, arch = model
    log = logging.getLogger("bench_mdxc_batch")
    log.setLevel(logging.ERROR)
    common = {"logger": log, "log_level": logging.ERROR, "torch_device": "cuda:0", "torch_device_cpu": "cpu", "torch_device_mps": None,
              "model_name": name, "model_path": name + ".ckpt", "model_data": cfg.as_model_data(), "asx_state_dict": sd,
              "output_format": "WAV", "output_bitrate": None, "output_dir": out_dir, "normalization_threshold": 0.9,
              "amplification_threshold": 0.0, "output_single_stem": None, "invert_using_spec": False, "sample_rate": SR,
              "use_soundfile": False}
    return MDXCSeparator(common_config=common, arch_config=dict(arch, segment_size=256, override_model_segment_size=False, batch_size=1,
                                                                pitch_shift=0))


def run(args):
    import numpy as np
    import torch
    from audio_separator_amd import audio_io
    from tools.bench_siblings import synth
    if not torch.cuda.is_available():
        sys.exit("bench_mdxc_batch.py: no GPU (there is no CPU path to time)")
    legs = args.legs.split(",")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for net in args.nets.split(","):
            dirs = {leg: os.path.join(tmp, net, leg) for leg in legs}
            model = make_model(net)
            seps = {leg: make_separator(model, d) for leg, d in dirs.items()}   # one resident model per leg: the output directory differs
            name = "rof_net_passes" if net == "rof" else "v3_net_passes"
            for w in args.workloads.split(","):
                songs, seconds, what = WORKLOADS[w]
                n = int(SR * seconds)
                first = synth(n)
                paths = []
                for s in range(songs):
                    p = os.path.join(tmp, f"{w}{s:02d}.wav")
                    audio_io.write_wav(p, np.clip(np.roll(first, 7919 * s, axis=1).T, -0.99, 0.99), SR, "PCM_16")
                    paths.append(p)

                def loop(sep):
                    out = []
                    for p in paths:
                        out.append(sep.separate(p))
                        sep.clear_file_specific_paths()
                    return out

                def pool(sep):
                    if not hasattr(sep, "separate_many"):
                        sys.exit("bench_mdxc_batch.py: this checkout has no MDXCSeparator.separate_many (run --legs loop)")
                    out = sep.separate_many(paths)
                    assert not sep.batch_errors, sep.batch_errors
                    return out
                steps = {"loop": loop, "pool": pool}
                # identity first (and the warm-up): the files of the two legs, byte for byte
                names = {leg: steps[leg](seps[leg]) for leg in legs}
                torch.cuda.synchronize()
                if len(legs) == 2:
                    assert names["loop"] == names["pool"] and all(len(x) == 2 for x in names["loop"]), "the legs name different files"
                    for per_file in names["loop"]:
                        for f in per_file:
                            assert filecmp.cmp(os.path.join(dirs["loop"], f), os.path.join(dirs["pool"], f), shallow=False), f"{f} differs"
                for leg in legs:
                    sep = seps[leg]
                    def counter():
                        try:
                            return sep.engine.counter(name)
                        except Exception:          # an earlier checkout has no such counter
                            return None
                    ms, net_passes = [], None
                    for _ in range(args.reps):
                        n0 = counter()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        steps[leg](sep)
                        torch.cuda.synchronize()
                        ms.append((time.perf_counter() - t0) * 1e3)
                        net_passes = counter() - n0 if n0 is not None else None
                    med = statistics.median(ms)
                    line = {"tool": "bench_mdxc_batch", "tag": args.tag, "net": net, "workload": w, "what": what, "leg": leg, "songs": songs,
                            "seconds_per_song": seconds, "reps": args.reps, "identical_files": len(legs) == 2,
                            "ms": [round(x, 2) for x in ms], "median_ms": round(med, 2), "spread": round(spread(ms), 5),
                            "audio_s_per_wall_s": round(songs * seconds / (med * 1e-3), 2)}
                    if net_passes is not None:
                        line["net_passes"] = net_passes
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                for p in paths:
                    os.remove(p)
            for sep in seps.values():
                sep.clear_gpu_cache()
                for dm in sep._demixers.values():
                    dm.engine.close()
            del seps, model
            torch.cuda.empty_cache()
            shutil.rmtree(os.path.join(tmp, net), ignore_errors=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def merge(args):
    """Lines of several runs -> one record: per (net, workload, tag / leg) every run's median, the median of those and the
    run-to-run spread; per (net, workload) the pooled call against the baseline's loop."""
    rows = []
    for path in args.merge:
        with open(path) as f:
            rows += [json.loads(line) for line in f if line.strip().startswith("{")]
    out = {"tool": "tools/bench_mdxc_batch.py",
           "metric": "wall time of one pass over the workload, files in and files out (device drained), ms; lower is better",
           "setting": "16-bit 44.1 kHz WAV inputs, device-resident file path, synthetic weights; " + "; ".join(f"{k}: {v}" for k, v in NETS.items()),
           "cases": {}}
    for net, w in sorted({(r["net"], r["workload"]) for r in rows}):
        mine = [r for r in rows if (r["net"], r["workload"]) == (net, w)]
        rec = {"what": WORKLOADS[w][2], "net": NETS[net], "legs": {}}
        for key in sorted({(r["tag"], r["leg"]) for r in mine}):
            runs = [r for r in mine if (r["tag"], r["leg"]) == key]
            meds = [r["median_ms"] for r in runs]
            leg = {"runs": len(runs), "run_medians_ms": meds, "median_ms": round(statistics.median(meds), 2),
                   "run_to_run_spread": round(spread(meds), 5) if len(meds) > 1 else None,
                   "within_run_spread_max": max(r["spread"] for r in runs), "reps_per_run": runs[0]["reps"],
                   "identical_files_checked": all(r.get("identical_files") for r in runs)}
            if "net_passes" in runs[-1]:
                leg["net_passes"] = runs[-1]["net_passes"]
            rec["legs"][f"{key[0]}/{key[1]}"] = leg
        legs = rec["legs"]
        for name, a, b in (("pool_over_baseline_loop", f"{args.feature_tag}/pool", f"{args.baseline_tag}/loop"),
                           ("loop_over_baseline_loop", f"{args.feature_tag}/loop", f"{args.baseline_tag}/loop"),
                           ("pool_over_loop", f"{args.feature_tag}/pool", f"{args.feature_tag}/loop")):
            if a in legs and b in legs:
                rec[name] = round(legs[a]["median_ms"] / legs[b]["median_ms"], 4)
        out["cases"][f"{net}/{w}"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="rof,mdx23c")
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--legs", default="loop,pool")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="this", help="names the checkout the run was made from in the merged record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--baseline-tag", default="parent")
    ap.add_argument("--feature-tag", default="this")
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.reps < 3:
        sys.exit("bench_mdxc_batch.py: at least 3 timed passes")
    run(args)


if __name__ == "__main__":
    main()
