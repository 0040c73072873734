#!/usr/bin/env python3
"""A batch of songs through the Demucs path: one pooled call (Engine.ht_demix_batch_dev / hd_demix_batch_dev) against the loop of
single-song calls (ht_demix_dev / hd_demix_dev).

    python tools/bench_demucs_batch.py [--nets ht,hd] [--workloads a,b] [--legs loop,pool] [--reps 5] [--warmup 1] [--tag NAME] [--out FILE]

Nets: the htdemucs layout (v4, 7.8-s segments) and the hdemucs_mmi layout (v3, 44-s chunks) with synthetic weights, as
tools/bench_siblings.py builds them.  shifts = 2 with fixed offsets (the same in both legs), overlap 0.25, flags 3 (standardise +
stem swap), every buffer resident in HBM, `warmup` passes per leg, then `reps` passes each timed with a pair of device events
around the calls; one JSON line per (net, workload, leg) with every pass, the median and the spread (max - min) / median.

  a   64 clips x 20 s   (v4: 8 segment-forwards each -- the loop runs 64 forwards of 8, the pool 16 of 32)
  b   8 songs x 4 min   (BASELINE config 5's share per rank; the loop's forwards are already full)

The leg `single` times ONE 4-minute song through the single-song call (it must not move when the pool is added).  The `loop` and
`single` legs need nothing this tool's commit added, so the same file run from a checkout of an earlier commit gives that commit's
baseline; `--merge` folds the lines of several runs into one record:

    python tools/bench_demucs_batch.py --merge run1.jsonl run2.jsonl ... --out profiles/NAME_demucs_batch_pool.json
"""
import argparse
import json
import os
import statistics
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 44100
WORKLOADS = {"a": (64, 20.0, "64 clips x 20 s"), "b": (8, 240.0, "8 songs x 4 min")}
OFFSETS = [11025, 3000]


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def synth(n, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = sum(rng.uniform(0.02, 0.1) * np.sin(2 * np.pi * rng.uniform(60, 8000) * t + rng.uniform(0, 6.28)) for _ in range(8))
    return (np.stack([x, 0.8 * x]) + 0.1 * rng.standard_normal((2, n))).astype(np.float32)


def make_engine(A, net):
    if net == "ht":
        from oracle import demucs_oracle as D
        eng = A.Engine(A.MDXConfig(n_fft=4096, hop_length=1024, dim_f=2048, segment_size=8))
        eng.load_ht(A.HTConfig(segment=Fraction(39, 5)), D.make_ht_state(D.HTConfig(), 0))
        return eng, "htdemucs layout (v4, 7.8-s segments)"
    from oracle import hdemucs_oracle as H
    eng = A.Engine(A.MDXConfig(n_fft=4096, hop_length=1024, dim_f=2048, segment_size=8))
    eng.load_hd(A.HDConfig(segment=44), H.make_hd_state(H.HDConfig(segment=44), 0))
    return eng, "hdemucs_mmi layout (v3, 44-s chunks)"


def run(args):
    import torch
    import audio_separator_amd as A
    if not torch.cuda.is_available():
        sys.exit("bench_demucs_batch.py: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for net in args.nets.split(","):
        eng, layout = make_engine(A, net)
        single = eng.ht_demix_dev if net == "ht" else eng.hd_demix_dev
        batch = getattr(eng, f"{net}_demix_batch_dev", None)
        plan = eng.ht_plan if net == "ht" else eng.hd_plan
        for w in args.workloads.split(","):
            songs, seconds, what = WORKLOADS[w]
            n = int(SR * seconds)
            first = torch.from_numpy(synth(n)).to(dev)
            mixes = [first] + [torch.roll(first, 7919 * s, dims=1).contiguous() for s in range(1, songs)]
            outs = [torch.empty((4, 2, n), dtype=torch.float32, device=dev) for _ in mixes]
            segments = plan(n, 2, OFFSETS, 0.25)["n_chunks"]

            def loop():
                for m, o in zip(mixes, outs):
                    single(m.data_ptr(), n, o.data_ptr(), shifts=2, offsets=OFFSETS, overlap=0.25, flags=3, stream=stream)

            def pool():
                batch([(m.data_ptr(), o.data_ptr(), n, OFFSETS) for m, o in zip(mixes, outs)], shifts=2, overlap=0.25, flags=3, stream=stream)

            def one():
                single(mixes[0].data_ptr(), n, outs[0].data_ptr(), shifts=2, offsets=OFFSETS, overlap=0.25, flags=3, stream=stream)

            for leg in args.legs.split(","):
                if leg == "pool" and batch is None:
                    sys.exit("bench_demucs_batch.py: this checkout has no demix_batch_dev for Demucs (run --legs loop)")
                if leg == "single" and w != "b":
                    continue
                step = {"loop": loop, "pool": pool, "single": one}[leg]
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
                n_songs = 1 if leg == "single" else songs
                line = {"tool": "bench_demucs_batch", "tag": args.tag, "net": net, "layout": layout, "workload": w, "what": what, "leg": leg,
                        "songs": n_songs, "seconds_per_song": seconds, "segments_per_song": segments, "shifts": 2, "offsets": OFFSETS,
                        "reps": args.reps, "warmup": args.warmup, "ms": [round(x, 3) for x in ms], "median_ms": round(med, 3),
                        "spread": round(spread(ms), 5), "audio_s_per_wall_s": round(n_songs * seconds / (med * 1e-3), 2)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            del mixes, outs, first
            torch.cuda.empty_cache()
        eng.close()
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
    out = {"tool": "tools/bench_demucs_batch.py",
           "metric": "wall time of one pass over the workload (device events around the calls), ms; lower is better",
           "setting": "shifts 2 with fixed offsets, overlap 0.25, flags 3, synthetic weights, device-resident buffers", "nets": {}}
    for net in sorted({r["net"] for r in rows}):
        out["nets"][net] = {"layout": next(r["layout"] for r in rows if r["net"] == net), "workloads": {}}
        for w in sorted({r["workload"] for r in rows if r["net"] == net}):
            mine = [r for r in rows if r["net"] == net and r["workload"] == w]
            rec = {"what": WORKLOADS[w][2], "legs": {}}
            for key in sorted({(r["tag"], r["leg"]) for r in mine}):
                runs = [r for r in mine if (r["tag"], r["leg"]) == key]
                meds = [r["median_ms"] for r in runs]
                rec["legs"][f"{key[0]}/{key[1]}"] = {"runs": len(runs), "run_medians_ms": meds, "median_ms": round(statistics.median(meds), 3),
                                                    "run_to_run_spread": round(spread(meds), 5) if len(meds) > 1 else None,
                                                    "within_run_spread_max": max(r["spread"] for r in runs), "reps_per_run": runs[0]["reps"],
                                                    "segments_per_song": runs[0]["segments_per_song"]}
            legs = rec["legs"]
            for name, a, b in (("pool_over_baseline_loop", f"{args.feature_tag}/pool", f"{args.baseline_tag}/loop"),
                               ("loop_over_baseline_loop", f"{args.feature_tag}/loop", f"{args.baseline_tag}/loop"),
                               ("single_over_baseline_single", f"{args.feature_tag}/single", f"{args.baseline_tag}/single")):
                if a in legs and b in legs:
                    rec[name] = round(legs[a]["median_ms"] / legs[b]["median_ms"], 4)
            out["nets"][net]["workloads"][w] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="ht,hd")
    ap.add_argument("--workloads", default="a,b")
    ap.add_argument("--legs", default="loop,pool,single")
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
        sys.exit("bench_demucs_batch.py: at least 5 timed passes")
    run(args)


if __name__ == "__main__":
    main()
