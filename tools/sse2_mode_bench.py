#!/usr/bin/env python3
"""What the SSE2 arithmetic (opt=1, SN_ARITH_SSE2) costs against the default arithmetic of the SAME library, on
device-resident frames (--frames 16: a small launch, a few workgroups; --frames 1024: the GPU full, as bench.py runs it): tools/sse2_mode_bench.py [--fmt Y8] [--w 3840] [--h 2160] [--frames 16] [--iters 30] [--rounds 3]
[--modes auto pool].  The two arithmetics are alternated `rounds` times; one JSON line per run."""
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
ap.add_argument("--fmt", default="Y8")
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--modes", nargs="*", default=["auto", "pool"])
ap.add_argument("--pattern", default="noise")
ap.add_argument("--only-opt", type=int, default=None, help="run one arithmetic only (for a counter pass under rocprofv3)")
args = ap.parse_args()
dev = torch.device("cuda:0")
clip = clip_format(args.fmt, args.w, args.h)
vt = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]
src = synth.frame(clip, args.pattern, seed=1)
n = args.frames
dsrc = [torch.from_numpy(p.view(vt)).to(dev).unsqueeze(0).repeat(n, 1, 1) for p in src]  # the same frame n times, built on the device
for rnd in range(args.rounds):
    for mode in args.modes:
        for opt in ((0, 1) if args.only_opt is None else (args.only_opt,)):
            with SangNom2(clip, max_batch=n, mode=mode, aa=48, aac=48, opt=opt, small_launches=capi.SN_SMALL_SWEEP) as flt:
                ddst = [torch.zeros_like(t) for t in dsrc]
                torch.cuda.synchronize()
                for _ in range(3):
                    flt.process_batch(dsrc, ddst, parity=[1] * n)
                flt.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    flt.process_batch(dsrc, ddst, parity=[1] * n)
                flt.synchronize()
                t = (time.perf_counter() - t0) / args.iters
                i = flt.info()
                print(json.dumps({"frame": f"{args.w}x{args.h} {args.fmt}", "mode": mode, "opt": opt, "round": rnd,
                                  "fused": bool(i.fused_frames), "frames_per_launch": n, "ms_per_launch": round(t * 1e3, 4),
                                  "frames_per_s": round(n / t, 1)}), flush=True)
