#!/usr/bin/env python3
"""What the SSE2 arithmetic (opt=1, SN_ARITH_SSE2) costs against the default arithmetic of the SAME library, on
device-resident frames (--frames 16: a small launch, a few workgroups; --frames 1024: the GPU full, as bench.py runs it): tools/sse2_mode_bench.py [--fmt Y8 Y16 YUV420P8 YUV420P16] [--w 3840] [--h 2160] [--frames 16] [--iters 30] [--rounds 3]
[--modes auto pool] [--sweeps].  --sweeps creates the opt=1 contexts with sn_policy.sse2_sweeps = 1 (sweeps for 9..16-bit and
shared-pool 4:2:0 / 4:2:2 clips too; without it those run on the pool kernels in that arithmetic).  The formats and the two
arithmetics are alternated `rounds` times; one JSON line per run."""
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
ap.add_argument("--fmt", nargs="+", default=["Y8"], help="one or more of Y8, Y16, YUV420P8, YUV420P16, ...")
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--modes", nargs="*", default=["auto", "pool"])
ap.add_argument("--pattern", default="noise")
ap.add_argument("--only-opt", type=int, default=None, help="run one arithmetic only (for a counter pass under rocprofv3)")
ap.add_argument("--sweeps", action="store_true", help="sn_policy.sse2_sweeps = 1 in the opt=1 contexts")
args = ap.parse_args()
dev = torch.device("cuda:0")
n = args.frames
dsrc = {}
for fmt in args.fmt:
    clip = clip_format(fmt, args.w, args.h)
    vt = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]
    src = synth.frame(clip, args.pattern, seed=1)
    dsrc[fmt] = [torch.from_numpy(p.view(vt)).to(dev).unsqueeze(0).repeat(n, 1, 1) for p in src]  # the same frame n times, built on the device
for rnd in range(args.rounds):
    for fmt in args.fmt:
        clip = clip_format(fmt, args.w, args.h)
        for mode in args.modes:
            for opt in ((0, 1) if args.only_opt is None else (args.only_opt,)):
                knob = 1 if args.sweeps and opt == 1 else 0
                with SangNom2(clip, max_batch=n, mode=mode, aa=48, aac=48, opt=opt, small_launches=capi.SN_SMALL_SWEEP, sse2_sweeps=knob) as flt:
                    ddst = [torch.zeros_like(t) for t in dsrc[fmt]]
                    torch.cuda.synchronize()
                    for _ in range(3):
                        flt.process_batch(dsrc[fmt], ddst, parity=[1] * n)
                    flt.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        flt.process_batch(dsrc[fmt], ddst, parity=[1] * n)
                    flt.synchronize()
                    t = (time.perf_counter() - t0) / args.iters
                    i = flt.info()
                    print(json.dumps({"frame": f"{args.w}x{args.h} {fmt}", "mode": mode, "opt": opt, "sse2_sweeps": knob, "round": rnd,
                                      "fused": bool(i.fused_frames), "frames_per_launch": n, "ms_per_launch": round(t * 1e3, 4),
                                      "frames_per_s": round(n / t, 1)}), flush=True)
