#!/usr/bin/env python3
"""A batch of songs: one pooled call (Engine.demix_batch_dev) against the loop of single-song calls (Engine.demix_dev).

    python tools/bench_batch.py [--workloads a,b] [--legs loop,pool] [--reps 5] [--warmup 1] [--tag NAME] [--out FILE]

HQ_3 geometry and synthetic weights (workload/synth.py), every buffer resident in HBM, one warm-up pass per leg, then `reps`
passes each timed with a pair of device events around the calls; one JSON line per (workload, leg) with every pass, the median
and the spread (max - min) / median.

  a   64 clips x 20 s   (6 chunks each: the loop runs 64 net passes of 6 chunks, the pool 6 of 64)
  b   8 songs x 4 min   (55 chunks each: BASELINE config 5's share per rank; the loop's batches are already full)

The first song of a workload is workload/synth.py's seeded song; the others are that song rolled by a different number of
samples each (distinct inputs of the same statistics -- timing does not depend on the content, and 64 seeded songs are a minute
of host time per process).  The `loop` leg needs nothing this tool's commit added, so the same file run from a checkout of an
earlier commit gives that commit's baseline; `--merge` folds the lines of several runs into one record:

    python tools/bench_batch.py --merge run1.jsonl run2.jsonl ... --out profiles/NAME_batch_pool.json
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


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def run(args):
    import torch
    import audio_separator_amd as A
    from workload import synth as O
    if not torch.cuda.is_available():
        sys.exit("bench_batch.py: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    d = O.NetDims()
    eng = A.Engine(A.MDXConfig(max_batch=args.max_batch), device=0)
    eng.load_net(A.NetConfig(), A.fold_convtdf_state(O.make_convtdf_state(d, seed=0), d.num_blocks, d.l))
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for w in args.workloads.split(","):
        songs, seconds, what = WORKLOADS[w]
        n = int(SR * seconds)
        first = torch.from_numpy(O.synth_mix(n, seed=0)).to(dev)
        mixes = [first] + [torch.roll(first, 7919 * s, dims=1).contiguous() for s in range(1, songs)]
        outs = [torch.empty_like(m) for m in mixes]
        chunks = eng.plan(n)["n_chunks"]

        def loop():
            for m, o in zip(mixes, outs):
                eng.demix_dev(m.data_ptr(), n, o.data_ptr(), stream=stream)

        def pool():
            eng.demix_batch_dev([(m.data_ptr(), o.data_ptr(), n) for m, o in zip(mixes, outs)], stream=stream)

        for leg in args.legs.split(","):
            if leg == "pool" and not hasattr(eng, "demix_batch_dev"):
                sys.exit("bench_batch.py: this checkout has no demix_batch_dev (run --legs loop)")
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
            line = {"tool": "bench_batch", "tag": args.tag, "workload": w, "what": what, "leg": leg, "songs": songs, "seconds_per_song": seconds,
                    "chunks_per_song": chunks, "max_batch": args.max_batch or 64, "reps": args.reps, "warmup": args.warmup,
                    "ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round(spread(ms), 5),
                    "audio_s_per_wall_s": round(songs * seconds / (med * 1e-3), 2)}
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
    """Lines of several runs -> one record: per (workload, tag / leg) every run's median, the median of those and the run-to-run
    spread; per workload the pooled call against the baseline's loop."""
    rows = []
    for path in args.merge:
        with open(path) as f:
            rows += [json.loads(line) for line in f if line.strip().startswith("{")]
    out = {"tool": "tools/bench_batch.py", "metric": "wall time of one pass over the workload (device events around the calls), ms; lower is better",
           "geometry": "UVR-MDX-NET-Inst_HQ_3 (n_fft 6144, hop 1024, dim_f 3072, segment 256), synthetic weights, device-resident buffers",
           "workloads": {}}
    for w in sorted({r["workload"] for r in rows}):
        rec = {"what": WORKLOADS[w][2], "legs": {}}
        for key in sorted({(r["tag"], r["leg"]) for r in rows if r["workload"] == w}):
            runs = [r for r in rows if r["workload"] == w and (r["tag"], r["leg"]) == key]
            meds = [r["median_ms"] for r in runs]
            rec["legs"][f"{key[0]}/{key[1]}"] = {"runs": len(runs), "run_medians_ms": meds, "median_ms": round(statistics.median(meds), 3),
                                                "run_to_run_spread": round(spread(meds), 5) if len(meds) > 1 else None,
                                                "within_run_spread_max": max(r["spread"] for r in runs), "reps_per_run": runs[0]["reps"],
                                                "chunks_per_song": runs[0]["chunks_per_song"]}
        base, pool = rec["legs"].get(f"{args.baseline_tag}/loop"), rec["legs"].get(f"{args.feature_tag}/pool")
        if base and pool:
            rec["pool_over_baseline_loop"] = round(pool["median_ms"] / base["median_ms"], 4)
        same = rec["legs"].get(f"{args.feature_tag}/loop")
        if base and same:
            rec["loop_over_baseline_loop"] = round(same["median_ms"] / base["median_ms"], 4)
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
    ap.add_argument("--max-batch", type=int, default=0)
    ap.add_argument("--tag", default="this", help="names the checkout the run was made from in the merged record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--baseline-tag", default="parent")
    ap.add_argument("--feature-tag", default="this")
    args = ap.parse_args()
    if args.merge:
        return merge(args)
    if args.reps < 5:
        sys.exit("bench_batch.py: at least 5 timed passes")
    run(args)


if __name__ == "__main__":
    main()
