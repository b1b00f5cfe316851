#!/usr/bin/env python3
"""What MSB-aligned surfaces (P010 / P012 as the 10- / 12-bit clips they are) cost on device-resident 2160p 4:2:0 batches,
against the LSB-aligned surface call of the SAME library and against the work-around a caller needed before the _MSB layouts
existed, in one process: tools/msb_surface_bench.py [--fmt YUV420P10] [--w 3840 --h 2160] [--frames 64] [--iters 10] [--rounds 3]
[--aac 48] [--pattern noise].

Per round, alternated, one JSON line each:
  p016        process_surfaces, SN_LAYOUT_SEMIPLANAR both sides, LSB-aligned data: the floor, no shift anywhere
  msb         process_surfaces, SN_LAYOUT_SEMIPLANAR_MSB both sides
  caller      the same pixels without the _MSB layouts: torch shifts of Y and UV down into LSB tensors (int16 >> is arithmetic,
              so masked after it), the p016 call, torch shifts of the output up; library and torch on one stream, no host waits
  shift_down  the plane passes alone, MSB in and LSB out through a context that processes nothing: the copied-plane conversion
  shift_up    ... LSB in and MSB out
  copy        a device-to-device copy of the frames (Y and UV tensors onto others): the yardstick
The summary line holds the two conditions of DESIGN.md 4.7 -- median(msb) <= median(caller) + spread(caller), and
median(msb) - median(p016) <= shift_down / 2 + shift_up + spread(p016) (the walk shifts down only the kept lines) -- the
msb / p016 ratio, and the two passes' rates in GB/s (bytes read plus bytes written) next to the copy's."""
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
ap.add_argument("--fmt", default="YUV420P10")
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
clip = clip_format(args.fmt, args.w, args.h)
assert clip.bytes == 2 and clip.bits < 16, "a 9..15-bit clip"
s, mask = 16 - clip.bits, (1 << clip.bits) - 1


def timed(call, sync):
    for _ in range(2):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        call()
    sync()
    return (time.perf_counter() - t0) / args.iters


fr = synth.frame(clip, args.pattern, seed=1)
planar = [torch.from_numpy(p.view(np.int16)).to(dev).unsqueeze(0).repeat(n, 1, 1) for p in fr]  # the same frame n times
lsb = [planar[0], torch.stack([planar[1], planar[2]], dim=-1).contiguous()]
del planar
low = [torch.randint(1, 1 << s, t.shape[1:], dtype=torch.int16, device=dev) for t in lsb]  # non-zero low bits, as a decoder may leave them
msb = [(t << s) | l for t, l in zip(lsb, low)]
out = [torch.zeros_like(t) for t in lsb]
out_msb = [torch.zeros_like(t) for t in lsb]
tmp = [torch.zeros_like(t) for t in lsb]       # the caller's LSB source
tmp_out = [torch.zeros_like(t) for t in lsb]   # ... and LSB output
frame_bytes = sum(t.numel() for t in lsb) * 2  # per launch
side = torch.cuda.Stream()
runs = {k: [] for k in ("p016", "msb", "caller", "shift_down", "shift_up", "copy")}

with SangNom2(clip, max_batch=n, aac=args.aac) as a, SangNom2(clip, max_batch=n, aac=args.aac) as b, \
        SangNom2(clip, max_batch=n, aac=args.aac, stream=side.cuda_stream) as c, SangNom2(clip, max_batch=n, luma=False, chroma=False) as idle:

    def caller():
        with torch.cuda.stream(side):
            for t, m in zip(tmp, msb):
                torch.bitwise_right_shift(m, s, out=t)
                t.bitwise_and_(mask)
            c.process_surfaces(tmp, tmp_out)
            for t, o in zip(tmp_out, out_msb):
                torch.bitwise_left_shift(t, s, out=o)

    a.process_surfaces(lsb, out)  # the first calls allocate the scratch
    b.process_surfaces(msb, out_msb, src_msb=True, dst_msb=True)
    b.synchronize()
    want = [t.clone() for t in out_msb]
    for t in out_msb:
        t.zero_()
    caller()
    side.synchronize()
    a.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, out_msb)), "the library and the work-around disagree"
    assert all(torch.equal(x, y << s) for x, y in zip(want, out)), "msb is not p016 shifted up"
    del want
    for rnd in range(args.rounds):
        t = {}
        t["p016"] = timed(lambda: a.process_surfaces(lsb, out), a.synchronize)
        t["msb"] = timed(lambda: b.process_surfaces(msb, out_msb, src_msb=True, dst_msb=True), b.synchronize)
        t["caller"] = timed(caller, side.synchronize)
        t["shift_down"] = timed(lambda: idle.process_surfaces(msb, out, src_msb=True), idle.synchronize)
        t["shift_up"] = timed(lambda: idle.process_surfaces(lsb, out_msb, dst_msb=True), idle.synchronize)
        t["copy"] = timed(lambda: [o.copy_(x) for o, x in zip(out, lsb)], torch.cuda.synchronize)
        for k, v in t.items():
            runs[k].append(v)
            print(json.dumps({"frame": f"{args.w}x{args.h} {args.fmt}", "what": k, "round": rnd, "frames_per_launch": n, "ms_per_launch": round(v * 1e3, 4),
                              "frames_per_s": round(n / v, 1) if k in ("p016", "msb", "caller") else None,
                              "gb_per_s": round(2 * frame_bytes / v / 1e9, 1) if k in ("shift_down", "shift_up", "copy") else None}), flush=True)
    assert idle.surface_info().scratch_bytes == 0
    scratch = (a.surface_info().scratch_bytes, b.surface_info().scratch_bytes)

med = {k: statistics.median(v) for k, v in runs.items()}
spread = {k: max(v) - min(v) for k, v in runs.items()}
extra = med["msb"] - med["p016"]
bound = med["shift_down"] / 2 + med["shift_up"] + spread["p016"]
print(json.dumps({"frame": f"{args.w}x{args.h} {args.fmt}", "what": "summary", "frames_per_launch": n,
                  "p016_frames_per_s": round(n / med["p016"], 1), "msb_frames_per_s": round(n / med["msb"], 1),
                  "caller_frames_per_s": round(n / med["caller"], 1), "msb_over_p016": round(med["msb"] / med["p016"], 4),
                  "msb_ms": round(med["msb"] * 1e3, 4), "caller_ms": round(med["caller"] * 1e3, 4), "caller_spread_ms": round(spread["caller"] * 1e3, 4),
                  "beats_caller": bool(med["msb"] <= med["caller"] + spread["caller"]),
                  "msb_minus_p016_ms": round(extra * 1e3, 4), "shift_down_ms": round(med["shift_down"] * 1e3, 4),
                  "shift_up_ms": round(med["shift_up"] * 1e3, 4), "p016_spread_ms": round(spread["p016"] * 1e3, 4), "bound_ms": round(bound * 1e3, 4),
                  "holds": bool(extra <= bound),
                  "shift_down_gb_per_s": round(2 * frame_bytes / med["shift_down"] / 1e9, 1), "shift_up_gb_per_s": round(2 * frame_bytes / med["shift_up"] / 1e9, 1),
                  "copy_gb_per_s": round(2 * frame_bytes / med["copy"] / 1e9, 1),
                  "scratch_mb_p016": round(scratch[0] / 2**20, 1), "scratch_mb_msb": round(scratch[1] / 2**20, 1)}), flush=True)
