#!/usr/bin/env python3
"""A batch of songs through the VR path: one pooled call (Engine.vr_separate_batch_dev) against the loop of single-song calls
(vr_separate_dev) over the same songs.

    python tools/bench_vr_batch.py [--workloads a,b] [--legs loop,pool] [--reps 5] [--warmup 1] [--tag NAME] [--out FILE]

Net: the 4band_44100 layout with the HP-size CascadedASPPNet (2_HP-UVR shape) and synthetic weights, window 512, as
tools/bench_siblings.py builds it; VRDemixer's default of 48 patches per pass, aggression 5, no TTA, both stems.  Every buffer is
resident in HBM; `warmup` passes per leg, then `reps` passes each timed with a pair of device events around the calls; one JSON
line per (workload, leg) with every pass, the median and the spread (max - min) / median.  The pooled leg adds the share of
its device time spent in the per-song analysis / synthesis launches (asx_profile_read classes stft, istft, ola; the class
misc is listed beside them: it holds the per-song resamplers AND the net's element-wise kernels), from one extra profiled pass.

  a   64 clips x 20 s   (7 patches each: the loop runs 64 passes of 7, the pool 10 of 45)
  b   8 songs x 4 min   (81 patches each: the loop runs 16 passes of 41 or 40, the pool 14 of 47 or 46)

The `loop` leg needs nothing this tool's commit added, so the same file run from a checkout of an earlier commit gives that
commit's baseline; `--merge` folds the lines of several runs into one record:

    python tools/bench_vr_batch.py --merge run1.jsonl run2.jsonl ... --out profiles/NAME_vr_batch_pool.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
WORKLOADS = {"a": (64, 20.0, "64 clips x 20 s"), "b": (8, 240.0, "8 songs x 4 min")}
PER_SONG_CLASSES = ("stft", "istft", "ola")   # launched per song only; "misc" mixes the per-song resamplers with the net's element-wise kernels


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def run(args):
    import torch
    import audio_separator_amd as A
    from oracle import vr_oracle as V
    from tools.bench_siblings import VR_MP, synth
    if not torch.cuda.is_available():
        sys.exit("bench_vr_batch.py: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    arch = 123821
    dm = A.VRDemixer({"model_params": VR_MP, "primary_stem_name": "Instrumental", "torch_device": 0},
                     {"window_size": 512, "batch_size": 8, "aggression": 5}, state_dict=V.make_vr_state(arch, 0), nn_arch_size=arch)
    eng = dm.engine
    batch = getattr(eng, "vr_separate_batch_dev", None)
    lines = []
    for w in args.workloads.split(","):
        songs, seconds, what = WORKLOADS[w]
        n = int(SR * seconds)
        frames, n_out = eng.vr_plan(n)
        first = torch.from_numpy(synth(n)).to(dev)
        waves = [first] + [torch.roll(first, 7919 * s, dims=1).contiguous() for s in range(1, songs)]
        outs = [torch.empty((2, 2, n_out), dtype=torch.float32, device=dev) for _ in waves]

        def loop():
            for x, o in zip(waves, outs):
                eng.vr_separate_dev(x.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr(), 0.05, 186, stream=stream)

        def pool():
            batch([(x.data_ptr(), n, o[0].data_ptr(), o[1].data_ptr()) for x, o in zip(waves, outs)], 0.05, 186, stream=stream)

        for leg in args.legs.split(","):
            if leg == "pool" and batch is None:
                sys.exit("bench_vr_batch.py: this checkout has no vr_separate_batch_dev (run --legs loop)")
            step = {"loop": loop, "pool": pool}[leg]
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            line = {"tool": "bench_vr_batch", "tag": args.tag, "workload": w, "what": what, "leg": leg, "songs": songs,
                    "seconds_per_song": seconds, "patches_per_song": frames // 256 + 1,
                    "reps": args.reps, "warmup": args.warmup, "ms": [round(x, 3) for x in ms], "median_ms": round(med, 3),
                    "spread": round(spread(ms), 5), "audio_s_per_wall_s": round(songs * seconds / (med * 1e-3), 2)}
            if hasattr(eng, "counter"):
                try:
                    n0 = eng.counter("vr_net_passes")
                    step()
                    line["net_passes"] = eng.counter("vr_net_passes") - n0
                except A.AsxError:
                    pass
            if leg == "pool":
                # one profiled pass: device time per launch class
                torch.cuda.synchronize()
                eng.profile_enable(True)
                step()
                prof = eng.profile_read()
                eng.profile_enable(False)
                total = sum(v["ms"] for v in prof.values())
                per_song = sum(prof[c]["ms"] for c in PER_SONG_CLASSES if c in prof)
                line["profiled_device_ms"] = {k: round(v["ms"], 3) for k, v in prof.items() if v["launches"]}
                line["profiled_launches"] = {k: int(v["launches"]) for k, v in prof.items() if v["launches"]}
                line["per_song_class_share"] = round(per_song / total, 4) if total else None
            print(json.dumps(line), flush=True)
            lines.append(line)
        del waves, outs, first
        torch.cuda.empty_cache()
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def merge(args):
    """Lines of several runs -> one record: per (workload, tag / leg) every run's median, the median of those and the run-to-run
    spread; per workload the pooled call against the baseline's loop."""
    rows = []
    for path in args.merge:
        with open(path) as f:
            rows += [json.loads(line) for line in f if line.strip().startswith("{")]
    out = {"tool": "tools/bench_vr_batch.py",
           "metric": "wall time of one pass over the workload (device events around the calls), ms; lower is better",
           "setting": "4band_44100 layout, HP-size net, window 512, 48 patches per pass, aggression 5, synthetic weights, device-resident buffers",
           "workloads": {}}
    for w in sorted({r["workload"] for r in rows}):
        mine = [r for r in rows if r["workload"] == w]
        rec = {"what": WORKLOADS[w][2], "legs": {}}
        for key in sorted({(r["tag"], r["leg"]) for r in mine}):
            runs = [r for r in mine if (r["tag"], r["leg"]) == key]
            meds = [r["median_ms"] for r in runs]
            leg = {"runs": len(runs), "run_medians_ms": meds, "median_ms": round(statistics.median(meds), 3),
                   "run_to_run_spread": round(spread(meds), 5) if len(meds) > 1 else None,
                   "within_run_spread_max": max(r["spread"] for r in runs), "reps_per_run": runs[0]["reps"],
                   "patches_per_song": runs[0]["patches_per_song"]}
            for extra in ("net_passes", "per_song_class_share", "profiled_device_ms", "profiled_launches"):
                if extra in runs[-1]:
                    leg[extra] = runs[-1][extra]
            rec["legs"][f"{key[0]}/{key[1]}"] = leg
        legs = rec["legs"]
        for name, a, b in (("pool_over_baseline_loop", f"{args.feature_tag}/pool", f"{args.baseline_tag}/loop"),
                           ("loop_over_baseline_loop", f"{args.feature_tag}/loop", f"{args.baseline_tag}/loop"),
                           ("pool_over_loop", f"{args.feature_tag}/pool", f"{args.feature_tag}/loop")):
            if a in legs and b in legs:
                rec[name] = round(legs[a]["median_ms"] / legs[b]["median_ms"], 4)
        out["workloads"][w] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--legs", default="loop,pool")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tag", default="this", help="names the checkout the run was made from in the merged record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--baseline-tag", default="parent")
    ap.add_argument("--feature-tag", default="this")
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.reps < 5:
        sys.exit("bench_vr_batch.py: at least 5 timed passes")
    run(args)


if __name__ == "__main__":
    main()
