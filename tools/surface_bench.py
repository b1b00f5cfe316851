#!/usr/bin/env python3
"""What semi-planar surfaces (NV12 / P016) cost on device-resident 2160p 4:2:0 batches, against the planar call of the SAME
library in the same process: tools/surface_bench.py [--fmts YUV420P8 YUV420P16] [--w 3840 --h 2160] [--frames 64] [--iters 10]
[--rounds 3] [--aac 48] [--pattern noise].

Per format and round, alternated, one JSON line each:
  planar      process_batch on planar tensors
  semi        process_surfaces, semi-planar in and out (kept-lines split, passes on the scratch, merge)
  split       the split launch alone, all lines: a context that processes nothing, semi-planar in and planar out, minus `luma`
  merge       the merge launch alone: the same context, planar in and semi-planar out, minus `luma`
  luma        what both of those also do: the luma plane copied by the frame assembly (a Y context that processes nothing)
  copy        a device-to-device copy of one frame's chroma bytes per frame (the UV tensor onto another): the yardstick
The summary line per format holds the condition of DESIGN.md 4.7: median(semi) - median(planar) against
split + merge (the call splits only the kept lines: split / 2 is reported as well) plus the spread of the planar runs,
and the split and merge rates in GB/s (bytes read plus bytes written) next to the copy's."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avisynth_sangnom2_amd import SangNom2, clip_format, synth

ap = argparse.ArgumentParser()
ap.add_argument("--fmts", nargs="*", default=["YUV420P8", "YUV420P16"])
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--aac", type=int, default=48)
ap.add_argument("--pattern", default="noise")
args = ap.parse_args()
dev = torch.device("cuda:0")
n = args.frames


def timed(call, sync):
    for _ in range(2):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        call()
    sync()
    return (time.perf_counter() - t0) / args.iters


for fmt in args.fmts:
    clip = clip_format(fmt, args.w, args.h)
    yclip = clip_format({1: "Y8", 2: "Y16"}[clip.bytes], args.w, args.h)
    vt = {1: np.uint8, 2: np.int16}[clip.bytes]
    fr = synth.frame(clip, args.pattern, seed=1)
    planar = [torch.from_numpy(p.view(vt)).to(dev).unsqueeze(0).repeat(n, 1, 1) for p in fr]  # the same frame n times
    semi = [planar[0], torch.stack([planar[1], planar[2]], dim=-1).contiguous()]
    out_planar = [torch.zeros_like(t) for t in planar]
    out_semi = [out_planar[0], torch.zeros_like(semi[1])]
    chroma_bytes = semi[1].numel() * clip.bytes  # per launch
    runs = {k: [] for k in ("planar", "semi", "split", "merge", "luma", "copy")}
    with SangNom2(clip, max_batch=n, aac=args.aac) as a, SangNom2(clip, max_batch=n, aac=args.aac) as b, \
            SangNom2(clip, max_batch=n, luma=False, chroma=False) as idle, SangNom2(yclip, max_batch=n, luma=False) as yidle:
        b.process_surfaces(semi, out_semi)  # the first semi-planar call allocates the scratch
        b.synchronize()
        for rnd in range(args.rounds):
            t = {}
            t["planar"] = timed(lambda: a.process_batch(planar, out_planar), a.synchronize)
            t["semi"] = timed(lambda: b.process_surfaces(semi, out_semi), b.synchronize)
            t["luma"] = timed(lambda: yidle.process_batch(planar[:1], out_planar[:1]), yidle.synchronize)
            t["split"] = timed(lambda: idle.process_surfaces(semi, out_planar), idle.synchronize) - t["luma"]
            t["merge"] = timed(lambda: idle.process_surfaces(planar, out_semi), idle.synchronize) - t["luma"]
            t["copy"] = timed(lambda: out_semi[1].copy_(semi[1]), torch.cuda.synchronize)
            for k, v in t.items():
                runs[k].append(v)
                print(json.dumps({"frame": f"{args.w}x{args.h} {fmt}", "what": k, "round": rnd, "frames_per_launch": n, "ms_per_launch": round(v * 1e3, 4),
                                  "frames_per_s": round(n / v, 1) if k in ("planar", "semi") else None,
                                  "gb_per_s": round(2 * chroma_bytes / v / 1e9, 1) if k in ("split", "merge", "copy") else None}), flush=True)
        si = b.surface_info()
        assert (si.split_frames, si.merged_frames) == ((2 + args.iters) * args.rounds * n + n,) * 2 and idle.surface_info().scratch_bytes == 0
    med = {k: statistics.median(v) for k, v in runs.items()}
    extra = med["semi"] - med["planar"]
    spread = max(runs["planar"]) - min(runs["planar"])
    bound = med["split"] + med["merge"] + spread
    print(json.dumps({"frame": f"{args.w}x{args.h} {fmt}", "what": "summary", "frames_per_launch": n,
                      "planar_frames_per_s": round(n / med["planar"], 1), "semi_frames_per_s": round(n / med["semi"], 1),
                      "semi_minus_planar_ms": round(extra * 1e3, 4), "split_all_lines_ms": round(med["split"] * 1e3, 4),
                      "split_kept_lines_est_ms": round(med["split"] * 0.5e3, 4), "merge_ms": round(med["merge"] * 1e3, 4),
                      "planar_spread_ms": round(spread * 1e3, 4), "bound_ms": round(bound * 1e3, 4), "holds": bool(extra <= bound),
                      "split_gb_per_s": round(2 * chroma_bytes / med["split"] / 1e9, 1), "merge_gb_per_s": round(2 * chroma_bytes / med["merge"] / 1e9, 1),
                      "copy_gb_per_s": round(2 * chroma_bytes / med["copy"] / 1e9, 1),
                      "copy_spread_gb_per_s": round(2 * chroma_bytes / min(runs["copy"]) / 1e9 - 2 * chroma_bytes / max(runs["copy"]) / 1e9, 1)}), flush=True)
    del planar, semi, out_planar, out_semi
    torch.cuda.empty_cache()
