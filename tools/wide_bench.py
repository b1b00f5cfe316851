#!/usr/bin/env python3
"""What the column parts (sn_options.column_parts = 1) gain over the pool path for 16-bit and float planes wider than one
workgroup of the sweeps holds, on device-resident frames of the SAME library: tools/wide_bench.py [--shapes Y16:4096x2160 ...]
[--frames 256 16] [--iters 10] [--rounds 3] [--pattern noise] [--force-parts N] [--w W --h H --fmt Y16].
Every shape runs with column_parts 0 and 1, alternated `rounds` times; --frames 16 runs with SN_SMALL_SWEEP (under
SN_SMALL_AUTO such a launch goes where it went before the option existed).  --force-parts N (with --w / --h / --fmt: one
shape) cuts a plane that fits one workgroup into N parts through the test hook and runs it against the whole-plane sweep --
3840 x 2160 Y16 whole against two forced parts answers whether two 4-wave workgroups beat one 8-wave workgroup.  One JSON
line per run; part_fallbacks is the count over the timed launches and their warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avisynth_sangnom2_amd import SangNom2, capi, clip_format, synth

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="*", default=["Y16:4096x2160", "Y32:4096x2160", "Y16:7680x4320", "Y16:8192x4320"])
ap.add_argument("--fmt", default="Y16")
ap.add_argument("--w", type=int, default=0)
ap.add_argument("--h", type=int, default=0)
ap.add_argument("--frames", type=int, nargs="+", default=[256, 16])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--pattern", default="noise")
ap.add_argument("--force-parts", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda:0")
shapes = [f"{args.fmt}:{args.w}x{args.h}"] if args.w and args.h else args.shapes
for shape in shapes:
    fmt, wh = shape.split(":")
    w, h = (int(x) for x in wh.split("x"))
    clip = clip_format(fmt, w, h)
    vt = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]
    plane = torch.from_numpy(synth.frame(clip, args.pattern, seed=1)[0].view(vt)).to(dev)
    for n in args.frames:
        src = [plane.unsqueeze(0).repeat(n, 1, 1)]  # the same frame n times, built on the device
        dst = [torch.zeros_like(src[0])]
        for rnd in range(args.rounds):
            for parts in (0, 1):
                # the whole-plane sweep of a plane that fits (--force-parts) needs the option too: it is the hook that differs
                with SangNom2(clip, max_batch=n, mode="auto", aa=48, column_parts=1 if (parts or args.force_parts) else 0,
                              small_launches=capi.SN_SMALL_SWEEP if n < 171 else capi.SN_SMALL_AUTO) as flt:
                    if parts and args.force_parts:
                        flt.debug_set_column_parts(args.force_parts, 0)
                    torch.cuda.synchronize()
                    for _ in range(2):
                        flt.process_batch(src, dst, parity=[1] * n)
                    flt.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        flt.process_batch(src, dst, parity=[1] * n)
                    flt.synchronize()
                    t = (time.perf_counter() - t0) / args.iters
                    i, pi = flt.info(), flt.parts_info()
                    print(json.dumps({"frame": f"{w}x{h} {fmt}", "column_parts": parts, "parts": pi.parts[0], "round": rnd, "frames_per_launch": n,
                                      "fused_frames": i.fused_frames, "part_frames": pi.part_frames, "part_fallbacks": pi.part_fallbacks,
                                      "ms_per_launch": round(t * 1e3, 3), "frames_per_s": round(n / t, 1),
                                      "gpixel_per_s": round(n * w * h / t / 1e9, 3)}), flush=True)
        del src, dst
    del plane
    torch.cuda.empty_cache()
