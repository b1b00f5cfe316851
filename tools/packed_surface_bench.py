#!/usr/bin/env python3
"""What packed 4:2:2 surfaces (YUY2, Y210, v210) cost on device-resident 2160p batches, against the planar call of the SAME
library, against the torch slicing a caller needed before the packed layouts existed, and against a device-to-device copy, in
one process: tools/packed_surface_bench.py [--w 3840 --h 2160] [--frames 64] [--iters 10] [--rounds 3] [--aac 48]
[--formats yuyv8,y210,v210].

Per format and round, alternated, one JSON line each:
  planar   process_batch on planar tensors: the floor
  packed   process_surfaces, the packed layout on both sides
  caller   (yuyv8, y210) the same pixels without the packed layouts: torch strided slices (and shifts) into planar tensors, the
           planar call, slices back; library and torch on one stream, no host waits
  pack     planar in, packed out through a context that processes nothing: the pack kernel alone, all lines
  repack   packed in, packed out through that context: the unpack kernel (all lines) and the pack kernel; unpack = repack - pack
  copy     a device-to-device copy of one packed batch onto another: the yardstick
The summary line holds the conditions of DESIGN.md 4.9: median(packed) - median(planar) <= unpack / 2 + pack + spread(planar)
(the walk unpacks only the lines the passes keep), and the rates of unpack and pack in GB/s (bytes read plus bytes written: the
packed bytes plus the planar bytes, each once) next to the copy's."""
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

FORMATS = {"yuyv8": ("YUV422P8", "yuyv", False), "y210": ("YUV422P10", "yuyv", True), "v210": ("YUV422P10", "v210", False)}
ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=3840)
ap.add_argument("--h", type=int, default=2160)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--aac", type=int, default=48)
ap.add_argument("--pattern", default="noise")
ap.add_argument("--formats", default="yuyv8,y210,v210")
args = ap.parse_args()
dev = torch.device("cuda:0")
n, w, h = args.frames, args.w, args.h


def timed(call, sync):
    for _ in range(2):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        call()
    sync()
    return (time.perf_counter() - t0) / args.iters


def pack_v210_torch(y, u, v):
    """int16 planes [H, W], [H, W / 2] x 2 (W a multiple of 6) -> int32 [H, 4 W / 6]; set-up only, not timed."""
    y, u, v = (t.to(torch.int32).reshape(t.shape[0], -1, k) for t, k in ((y, 6), (u, 3), (v, 3)))
    words = torch.stack([u[..., 0] | y[..., 0] << 10 | v[..., 0] << 20, y[..., 1] | u[..., 1] << 10 | y[..., 2] << 20,
                         v[..., 1] | y[..., 3] << 10 | u[..., 2] << 20, y[..., 4] | v[..., 2] << 10 | y[..., 5] << 20], dim=-1)
    return words.reshape(words.shape[0], -1).contiguous()


for name in args.formats.split(","):
    fmt, layout, msb = FORMATS[name]
    clip = clip_format(fmt, w, h)
    s = 16 - clip.bits if msb else 0
    what = f"{w}x{h} {fmt} {name}"
    fr = synth.frame(clip, args.pattern, seed=1)
    vt = {1: np.uint8, 2: np.int16}[clip.bytes]
    planes = [torch.from_numpy(p.view(vt)).to(dev) for p in fr]
    if layout == "v210":
        assert w % 6 == 0
        one = pack_v210_torch(*planes)
    else:
        one = torch.empty((h, 2 * w), dtype=planes[0].dtype, device=dev)
        one[:, 0::2], one[:, 1::4], one[:, 3::4] = (p << s for p in planes)
    planar = [p.unsqueeze(0).repeat(n, 1, 1) for p in planes]  # the same frame n times
    packed = one.unsqueeze(0).repeat(n, 1, 1)
    del planes, one
    out_planar = [torch.zeros_like(t) for t in planar]
    out_packed, out_caller = torch.zeros_like(packed), torch.zeros_like(packed)
    tmp, tmp_out = [torch.zeros_like(t) for t in planar], [torch.zeros_like(t) for t in planar]
    packed_bytes = packed.numel() * packed.element_size()
    planar_bytes = sum(t.numel() * t.element_size() for t in planar)
    side = torch.cuda.Stream()
    kw = dict(src_packed=layout, dst_packed=layout, src_msb=msb, dst_msb=msb)
    kinds = ("planar", "packed") + (("caller",) if layout != "v210" else ()) + ("pack", "repack", "copy")
    runs = {k: [] for k in kinds}
    with SangNom2(clip, max_batch=n, aac=args.aac) as a, SangNom2(clip, max_batch=n, aac=args.aac) as b, \
            SangNom2(clip, max_batch=n, aac=args.aac, stream=side.cuda_stream) as c, SangNom2(clip, max_batch=n, luma=False, chroma=False) as idle:

        def caller():
            with torch.cuda.stream(side):
                for t, sl in zip(tmp, (packed[:, :, 0::2], packed[:, :, 1::4], packed[:, :, 3::4])):
                    if s:
                        torch.bitwise_right_shift(sl, s, out=t)
                        t.bitwise_and_((1 << clip.bits) - 1)
                    else:
                        t.copy_(sl)
                c.process_batch(tmp, tmp_out)
                for t, sl in zip(tmp_out, (out_caller[:, :, 0::2], out_caller[:, :, 1::4], out_caller[:, :, 3::4])):
                    sl.copy_(t << s if s else t)

        a.process_batch(planar, out_planar)
        b.process_surfaces(packed, out_packed, **kw)  # the first call allocates the scratch
        b.synchronize()
        a.synchronize()
        if layout != "v210":
            caller()
            side.synchronize()
            assert torch.equal(out_caller, out_packed), "the library and the work-around disagree"
        idle.process_surfaces(packed, out_caller, **kw)
        idle.synchronize()
        assert torch.equal(out_caller, packed), "a context that processes nothing must hand the frames through"
        for rnd in range(args.rounds):
            t = {}
            t["planar"] = timed(lambda: a.process_batch(planar, out_planar), a.synchronize)
            t["packed"] = timed(lambda: b.process_surfaces(packed, out_packed, **kw), b.synchronize)
            if "caller" in runs:
                t["caller"] = timed(caller, side.synchronize)
            t["pack"] = timed(lambda: idle.process_surfaces(planar, out_packed, dst_packed=layout, dst_msb=msb), idle.synchronize)
            t["repack"] = timed(lambda: idle.process_surfaces(packed, out_packed, **kw), idle.synchronize)
            t["copy"] = timed(lambda: out_packed.copy_(packed), torch.cuda.synchronize)
            for k, v in t.items():
                runs[k].append(v)
                print(json.dumps({"frame": what, "what": k, "round": rnd, "frames_per_launch": n, "ms_per_launch": round(v * 1e3, 4),
                                  "frames_per_s": round(n / v, 1) if k in ("planar", "packed", "caller") else None}), flush=True)
        scratch = b.surface_info().scratch_bytes
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    unpack = med["repack"] - med["pack"]
    extra, bound = med["packed"] - med["planar"], unpack / 2 + med["pack"] + spread["planar"]
    moved = packed_bytes + planar_bytes  # what one unpack or one pack reads plus writes
    line = {"frame": what, "what": "summary", "frames_per_launch": n, "planar_frames_per_s": round(n / med["planar"], 1),
            "packed_frames_per_s": round(n / med["packed"], 1), "packed_over_planar": round(med["packed"] / med["planar"], 4),
            "packed_minus_planar_ms": round(extra * 1e3, 4), "unpack_ms": round(unpack * 1e3, 4), "pack_ms": round(med["pack"] * 1e3, 4),
            "planar_spread_ms": round(spread["planar"] * 1e3, 4), "bound_ms": round(bound * 1e3, 4), "holds": bool(extra <= bound),
            "unpack_gb_per_s": round(moved / unpack / 1e9, 1), "pack_gb_per_s": round(moved / med["pack"] / 1e9, 1),
            "copy_gb_per_s": round(2 * packed_bytes / med["copy"] / 1e9, 1), "copy_spread_ms": round(spread["copy"] * 1e3, 4),
            "scratch_mb": round(scratch / 2**20, 1)}
    if "caller" in med:
        line.update(caller_frames_per_s=round(n / med["caller"], 1), beats_caller=bool(med["packed"] <= med["caller"] + spread["caller"]))
    print(json.dumps(line), flush=True)
    del planar, packed, out_planar, out_packed, out_caller, tmp, tmp_out
    torch.cuda.empty_cache()
