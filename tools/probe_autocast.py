#!/usr/bin/env python3
"""What the single-product arithmetic (engine option "gemm_f16x1", plugin knob ``asx_autocast``) gains on the Roformer demix: one 4-minute
44.1 kHz song in HBM through ``Engine.rof_demix_dev`` (device buffers: no file, no host copy in the timed part) on the BS-Roformer ep_317
layout and on a Mel-Band Roformer layout (dim 384, depth 6, 60 bands -- the published vocals model's), synthetic weights.  The option is
switched off and on ALTERNATELY in one process: two warm-up calls of either setting, then five timed pairs; per setting the median and the
spread (max - min) of the five wall times, then one profiled call each for the per-class device times of asx_profile_read (row GEMM =
"tdf", attention).  One JSON line per layout.

``--tree`` names the checkout whose package is measured (default: the one this file is in); a tree whose library does not know the option is
timed with the option off only -- the parent commit's forward, in the same job, to show that the default path did not move:

    python tools/probe_autocast.py [--nets rof,mel] [--seconds 240] [--calls 5] [--tree /path/to/another/checkout] [--label "parent commit"]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

SR = 44100
NETS = {"rof": "BS-Roformer ep_317 layout (dim 512, depth 12, 62 bands), step = chunk, 16 chunks per pass",
        "mel": "Mel-Band Roformer layout (dim 384, depth 6, 60 mel bands), step = chunk, 16 chunks per pass"}


def make_model(net):
    from oracle import roformer_oracle as R
    if net == "rof":
        cfg = R.RoformerConfig(freqs_per_bands=R.DEFAULT_FREQS_PER_BANDS)
    else:
        cfg = R.RoformerConfig.mel_config(dim=384, depth=6, num_bands=60, mask_estimator_depth=2)
    return cfg, R.make_roformer_state(cfg, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="rof,mel")
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--tree", default=here)
    ap.add_argument("--label", default=None, help="what the record calls the measured tree (default: its path)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.append(here)                                      # the oracle's seeded weights, where the measured tree is only the package
    import torch
    import audio_separator_amd as A
    from tools.bench_siblings import synth
    if not torch.cuda.is_available():
        sys.exit("probe_autocast.py: no GPU (there is no CPU path to time)")
    n = int(SR * args.seconds)
    mix = torch.from_numpy(synth(n)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for net in args.nets.split(","):
        cfg, sd = make_model(net)
        dm = A.MDXCDemixer({"model_data": cfg.as_model_data(), "torch_device": 0, "secondary_stem_name": cfg.instruments[1]},
                           {"overlap": 8}, state_dict=sd, max_batch=16)
        eng = dm.engine
        step = dm.roformer_step()
        out = torch.empty((int(eng.rof_cfg.n_out), 2, n), dtype=torch.float32, device="cuda")
        try:
            eng.set_option("gemm_f16x1", 0)
            settings = (0, 1)
        except A.AsxError:                                     # a library from before the option: the default path only
            settings = (0,)

        def call(on):
            if len(settings) > 1:
                eng.set_option("gemm_f16x1", on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.rof_demix_dev(mix.data_ptr(), n, step, out.data_ptr(), stream=st)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        walls = {on: [] for on in settings}
        results = {}
        for i in range(args.warmup + args.calls):
            for on in settings:                                # alternating: off, on, off, on, ...
                w = call(on)
                if i >= args.warmup:
                    walls[on].append(w)
                if i == args.warmup - 1:
                    results[on] = out.clone()
        classes = {}
        for on in settings:
            eng.profile_enable(True)
            call(on)
            prof = eng.profile_read()
            eng.profile_enable(False)
            classes[on] = {k: round(v["ms"], 2) for k, v in prof.items() if v["launches"]}
        rec = {"probe": "autocast", "tree": args.label or os.path.abspath(args.tree), "net": net, "what": NETS[net], "seconds": args.seconds,
               "calls": args.calls, "warmup": args.warmup}
        for on in settings:
            key = "on" if on else "off"
            rec[f"ms_{key}"] = round(1e3 * statistics.median(walls[on]), 2)
            rec[f"spread_{key}_ms"] = round(1e3 * (max(walls[on]) - min(walls[on])), 2)
            rec[f"x_realtime_{key}"] = round(args.seconds / statistics.median(walls[on]), 1)
            rec[f"class_ms_{key}"] = classes[on]
        if len(settings) > 1:
            rec["ratio_off_over_on"] = round(rec["ms_off"] / rec["ms_on"], 3)
            rec["faster_beyond_spread"] = bool(rec["ms_off"] - rec["ms_on"] > max(rec["spread_off_ms"], rec["spread_on_ms"]))
            a, b = results[1].double(), results[0].double()
            rec["rel_rms_on_vs_off"] = float(torch.sqrt(torch.mean((a - b) ** 2)) / torch.sqrt(torch.mean(b ** 2)))
        print(json.dumps(rec), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
