#!/usr/bin/env python3
"""Device-resident rate of the anti-aliasing idiom TurnLeft().SangNom2().TurnRight().SangNom2() (SangNomAA) and of
the turn kernel alone; with --host, frames from pageable host memory: the synchronous call (SangNomAAHost.get_frame)
against the ring at --depth.  --dh: the enlargement form (both passes with dh=true, destinations twice as wide and twice
as high); --dh --composed: the same idiom composed by hand from two SangNom2(dh=True) contexts and SangNom2.turn on one
stream, the way a caller had to build it before the call took dh.  --reduce tent|halfband (implies --dh): the enlarged
frame is reduced on the device, destinations of source size (device batches and --host).  --reduce-bw: the reduce kernel
alone (sn_reduce_device, both tap sets) against the turn kernel on the same 2W x 2H planes, alternating, --size being the
SOURCE size; any of Y8 / Y16 / Y32.  --mask lo,hi[,expand] (at source size: without --dh, or with --reduce): the call with
the edge mask next to the call without it, in one run (device batches and --host).  --mask-bw: the mask kernel alone
(sn_mask_merge_device, on noise -- every sample of the result is read -- and on a constant plane -- none is) against the
half-band reduce kernel that writes the same plane, alternating; any of Y8 / Y16 / Y32 -- and the luma-derived chroma merge
of a 4:2:0 frame of that size (sn_mask_merge_luma_device: U and V in one launch, in two launches) against the two own-mask
merges of the same chroma planes.  --mask-chroma luma (with --mask): the masked call merges chroma through luma's mask.
--sharpen AMOUNT (at source size; device batches): the call with the contra-sharpening (on top of --mask where given) next to
the call without it.  --sharpen-bw: the sharpening kernel alone (sn_contra_sharpen_device) against the mask kernel (expand 1, not
in place), both on noise and moving the same 3 W H B bytes per frame, alternating; any of Y8 / Y16 / Y32.
--fields both (without --dh; device batches): the call with both fields per pass next to the one-field call, alternating, with
the ratio of their medians (on top of --mask / --sharpen where given).  --merge-bw: the averaging kernel alone (sn_merge_device)
against the mask kernel (expand 1), both on noise and moving 3 W H B bytes per frame, and the turn of the average
(sn_turn_merge_device, 3 W H B) against the turn (2 W H B), alternating; any of Y8 / Y16 / Y32.
--repair K (1..4; at source size; device batches): the call with the rank repair (on top of --mask / --sharpen where given)
next to the call without it; --repair-chroma: every processed plane.  --repair-bw: the repair kernel alone (sn_repair_device,
ranks 1..4, and rank --repair or 1 in place) against the mask kernel (expand 1) and the sharpening kernel, all on noise and
moving the same 3 W H B bytes per frame, alternating; any of Y8 / Y16 / Y32.
usage: python tools/aa_bench.py [--frames 512] [--fresh 1] [--fmt Y8] [--size 3840x2160] [--dh [--composed]] [--reduce K] [--host [--depth 8]]
       python tools/aa_bench.py --reduce-bw [--fmt Y16] [--size 1920x1080] [--frames 64]
       python tools/aa_bench.py --mask 8,32,1 [--reduce halfband] [--size 1920x1080] [--host]
       python tools/aa_bench.py --mask-bw [--fmt Y16] [--size 3840x2160] [--frames 32]
       python tools/aa_bench.py --sharpen 64 --mask 8,32,1 --reduce halfband [--fmt YUV420P8]
       python tools/aa_bench.py --sharpen-bw [--fmt Y16] [--size 3840x2160] [--frames 256] [--reps 5]
       python tools/aa_bench.py --fields both [--fmt YUV420P8] [--size 1920x1080] [--frames 256] [--reps 9]
       python tools/aa_bench.py --merge-bw [--fmt Y16] [--size 3840x2160] [--frames 256] [--reps 9]
       python tools/aa_bench.py --repair 2 --mask 8,32,1 [--reduce halfband] [--fmt YUV420P8] [--frames 64]
       python tools/aa_bench.py --repair-bw [--fmt Y16] [--size 3840x2160] [--frames 256] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import numpy as np  # noqa: E402

from avisynth_sangnom2_amd import ClipFormat, SangNom2, SangNomAA, SangNomAAHost, clip_format  # noqa: E402


def host_rates(clip, a, mask_kw=None):
    """Frames from pageable host memory, every result collected into pageable memory: frames/s of the synchronous call and
    of the ring with as many frames in flight as it holds.  A whole frame crosses PCIe each way."""
    rng = np.random.default_rng(1)
    n = min(a.frames, 64)
    shapes = [(clip.height >> (clip.subh if p else 0), clip.width >> (clip.subw if p else 0)) for p in range(clip.planes)]
    frames = [[rng.integers(0, 256, s, dtype=np.uint8) for s in shapes] for _ in range(8)]
    out = {"clip": f"{clip.width}x{clip.height} planes {clip.planes}", "host_frames": n, "fresh_pool": bool(a.fresh)}
    up = sum(s[0] * s[1] for s in shapes) * clip.bytes
    if a.dh:
        out["dh"] = True
        out["pcie_bytes_per_frame_up"], out["pcie_bytes_per_frame_down"] = up, up if a.reduce else 4 * up
        if a.reduce:
            out["reduce"] = a.reduce
    else:
        out["pcie_bytes_per_frame_each_way"] = up
    dh_kw = dict(dh=True, **(dict(reduce=a.reduce) if a.reduce else {})) if a.dh else {}
    dh_kw.update(mask_kw or {})
    oshapes = [(2 * s[0], 2 * s[1]) if a.dh and not a.reduce else s for s in shapes]
    with SangNomAAHost(clip, aac=48 if clip.planes > 1 else 0, fresh_pool=bool(a.fresh), **dh_kw) as flt:
        for i in range(3):
            flt.get_frame(frames[i])
        t0 = time.perf_counter()
        for i in range(n):
            flt.get_frame(frames[i % 8])
        out["sync_fps"] = round(n / (time.perf_counter() - t0), 1)
    if not hasattr(SangNomAAHost, "submit"):
        return out
    with SangNomAAHost(clip, aac=48 if clip.planes > 1 else 0, fresh_pool=bool(a.fresh), host_depth=a.depth, **dh_kw) as flt:
        slots = flt.slots()
        dst = [np.zeros(s, np.uint8) for s in oshapes]

        def run(count):
            pending, f, done = [], 0, 0
            while done < count:
                while f < count and len(pending) < slots:
                    pending.append(flt.submit(frames[f % 8]))
                    f += 1
                flt.collect(pending.pop(0), dst)
                done += 1
        run(2 * slots)
        t0 = time.perf_counter()
        run(n)
        out["ring_fps"] = round(n / (time.perf_counter() - t0), 1)
        out["ring_slots"] = slots
    return out


def composed_dh_rate(clip, a, src, dst):
    """The dh idiom from two SangNom2(dh=True) contexts and SangNom2.turn on one stream: frames/s, device-resident."""
    N, dev = a.frames, src[0].device
    turned = ClipFormat(width=clip.height, height=clip.width, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subh, subh=clip.subw)
    wide = ClipFormat(width=2 * clip.width, height=clip.height, bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh)
    kw = dict(max_batch=N, fresh_pool=bool(a.fresh), aac=48 if clip.planes > 1 else 0, dh=True)
    with SangNom2(turned, **kw) as first, SangNom2(wide, stream=first.stream_handle(), **kw) as second:
        hw = [tuple(s.shape[1:]) for s in src]
        t1 = [torch.empty((N, w_, h_), device=dev, dtype=torch.uint8) for h_, w_ in hw]
        u1 = [torch.empty((N, 2 * w_, h_), device=dev, dtype=torch.uint8) for h_, w_ in hw]
        t2 = [torch.empty((N, h_, 2 * w_), device=dev, dtype=torch.uint8) for h_, w_ in hw]
        torch.cuda.synchronize()

        def once():
            for p in range(clip.planes):
                first.turn(src[p], t1[p], -1)
            first.process_batch(t1, u1)
            for p in range(clip.planes):
                first.turn(u1[p], t2[p], +1)
            second.process_batch(t2, dst)
        for _ in range(2):
            once()
        second.synchronize()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            once()
        second.synchronize()
        return round(N * reps / (time.perf_counter() - t0), 1)


def reduce_bandwidth(clip, a):
    """sn_reduce_device against sn_turn_device on the same planes E (2W x 2H, distinct frames), alternating: median seconds
    per launch of --frames frames; reduce moves 5 W H B bytes per frame (4 read, 1 written), the turn 8 W H B."""
    dev = torch.device("cuda:0")
    N, W, H, B = a.frames, clip.width, clip.height, clip.bytes
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[B]
    E = torch.randint(0, 256, (N, 2 * H, 2 * W * B), device=dev, dtype=torch.uint8).view(dt) if B != 4 else torch.rand((N, 2 * H, 2 * W), device=dev)
    turned = torch.empty((N, 2 * W, 2 * H), device=dev, dtype=dt)
    small = torch.empty((N, H, W), device=dev, dtype=dt)
    out = {"clip": f"{a.fmt} source {W}x{H}, E {2 * W}x{2 * H}", "frames": N, "E_bytes": N * 4 * W * H * B}
    with SangNom2(clip, max_batch=1) as flt:
        runs = {"turn": lambda: flt.turn(E, turned, 1), "tent": lambda: flt.reduce(E, small, "tent", 1, 0),
                "halfband": lambda: flt.reduce(E, small, "halfband", 1, 0)}
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        for r in range(a.reps + 1):
            for k, fn in runs.items():
                flt.synchronize()
                t0 = time.perf_counter()
                fn()
                flt.synchronize()
                if r:
                    times[k].append(time.perf_counter() - t0)
        for k, t in times.items():
            t.sort()
            moved = (8 if k == "turn" else 5) * N * W * H * B
            out[k + "_ms"] = round(1e3 * t[len(t) // 2], 3)
            out[k + "_GBps"] = round(moved / t[len(t) // 2] / 1e9, 1)
            out[k + "_GBps_min_max"] = [round(moved / t[-1] / 1e9, 1), round(moved / t[0] / 1e9, 1)]
    return out


def mask_bandwidth(clip, a):
    """sn_mask_merge_device (in place on the result, as the call uses it; expand 0 and 1) against the half-band sn_reduce_device
    that writes the same W x H plane, alternating: median seconds per launch of --frames frames.  The merge moves 3 W H B bytes
    per frame on noise (S and R read, dst written) and 2 W H B on a constant plane (R is not read where the mask is empty),
    the reduction 5 W H B."""
    dev = torch.device("cuda:0")
    N, W, H, B = a.frames, clip.width, clip.height, clip.bytes
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[B]

    def noise(h, w):
        if B == 4:
            return torch.rand((N, h, w), device=dev)
        hi = 1 << clip.bits
        return torch.randint(0, hi, (N, h, w), device=dev, dtype=torch.int32).to(dt)
    E, S, R = noise(2 * H, 2 * W), noise(H, W), noise(H, W)
    flat = torch.full((N, H, W), 0.3 if B == 4 else 77, device=dev, dtype=dt)
    small = torch.empty((N, H, W), device=dev, dtype=dt)
    lo, hi, _ = a.mask_values
    out = {"clip": f"{a.fmt} {W}x{H}", "frames": N, "plane_bytes": N * W * H * B, "mask": [lo, hi]}
    with SangNom2(clip, max_batch=1) as flt:
        runs = {"halfband": (5, lambda: flt.reduce(E, small, "halfband", 1, 0)),
                "mask0_noise": (3, lambda: flt.mask_merge(S, R, R, lo, hi, 0)), "mask1_noise": (3, lambda: flt.mask_merge(S, R, R, lo, hi, 1)),
                "mask1_flat": (2, lambda: flt.mask_merge(flat, R, R, lo, hi, 1)), "mask1_only": (2, lambda: flt.mask_merge(S, None, small, lo, hi, 1))}
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        for r in range(a.reps + 1):
            for k, (_, fn) in runs.items():
                flt.synchronize()
                t0 = time.perf_counter()
                fn()
                flt.synchronize()
                if r:
                    times[k].append(time.perf_counter() - t0)
        for k, t in times.items():
            t.sort()
            moved = runs[k][0] * N * W * H * B
            out[k + "_us_per_frame"] = round(1e6 * t[len(t) // 2] / N, 2)
            out[k + "_GBps"] = round(moved / t[len(t) // 2] / 1e9, 1)
            out[k + "_us_min_max"] = [round(1e6 * t[0] / N, 2), round(1e6 * t[-1] / N, 2)]
    out.update(luma_merge_times(clip, a, dev, dt, noise))
    return out


def sharpen_bandwidth(clip, a):
    """sn_contra_sharpen_device against sn_mask_merge_device (expand 1, into a third plane), both on noise, alternating: median,
    minimum and maximum microseconds per frame over --reps launches of --frames frames.  Both read S and R and write dst:
    3 W H B bytes per frame; `of_hbm_peak` is that over 8 TB/s over the median."""
    dev = torch.device("cuda:0")
    N, W, H, B = a.frames, clip.width, clip.height, clip.bytes
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[B]

    def noise():
        if B == 4:
            return torch.rand((N, H, W), device=dev)
        return torch.randint(0, 1 << clip.bits, (N, H, W), device=dev, dtype=torch.int32).to(dt)
    S, R = noise(), noise()
    dst = torch.empty((N, H, W), device=dev, dtype=dt)
    lo, hi, _ = a.mask_values
    amount = a.sharpen or 64
    out = {"clip": f"{a.fmt} {W}x{H}", "frames": N, "plane_bytes": N * W * H * B, "mask": [lo, hi, 1], "sharpen": amount, "reps": a.reps}
    with SangNom2(clip, max_batch=1) as flt:
        runs = {"sharpen": lambda: flt.contra_sharpen(S, R, dst, amount), "mask1": lambda: flt.mask_merge(S, R, dst, lo, hi, 1)}
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        for r in range(a.reps + 1):
            for k, fn in runs.items():
                flt.synchronize()
                t0 = time.perf_counter()
                fn()
                flt.synchronize()
                if r:
                    times[k].append(time.perf_counter() - t0)
        for k, t in times.items():
            t.sort()
            med = t[len(t) // 2]
            out[k + "_us_per_frame"] = round(1e6 * med / N, 2)
            out[k + "_us_min_max"] = [round(1e6 * t[0] / N, 2), round(1e6 * t[-1] / N, 2)]
            out[k + "_GBps"] = round(3 * N * W * H * B / med / 1e9, 1)
            out[k + "_of_hbm_peak"] = round(3 * N * W * H * B / 8e12 / med, 3)
    return out


def repair_bandwidth(clip, a):
    """sn_repair_device at every rank (and in place on R at rank --repair or 1) against sn_mask_merge_device (expand 1, into a
    third plane) and sn_contra_sharpen_device, all on noise, alternating: median, minimum and maximum microseconds per frame over
    --reps launches of --frames frames.  All read S and R and write dst: 3 W H B bytes per frame; `of_hbm_peak` is that over
    8 TB/s over the median."""
    dev = torch.device("cuda:0")
    N, W, H, B = a.frames, clip.width, clip.height, clip.bytes
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[B]

    def noise():
        if B == 4:
            return torch.rand((N, H, W), device=dev)
        return torch.randint(0, 1 << clip.bits, (N, H, W), device=dev, dtype=torch.int32).to(dt)
    S, R = noise(), noise()
    dst = torch.empty((N, H, W), device=dev, dtype=dt)
    lo, hi, _ = a.mask_values
    amount = a.sharpen or 64
    out = {"clip": f"{a.fmt} {W}x{H}", "frames": N, "plane_bytes": N * W * H * B, "mask": [lo, hi, 1], "sharpen": amount, "reps": a.reps}
    with SangNom2(clip, max_batch=1) as flt:
        runs = {"mask1": lambda: flt.mask_merge(S, R, dst, lo, hi, 1), "sharpen": lambda: flt.contra_sharpen(S, R, dst, amount)}
        for rank in (1, 2, 3, 4):
            runs[f"repair{rank}"] = lambda rank=rank: flt.repair(S, R, dst, rank)
        runs["repair_in_place"] = lambda: flt.repair(S, dst, dst, a.repair or 1)  # (on the last rank's output: the same traffic)
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        for r in range(a.reps + 1):
            for k, fn in runs.items():
                flt.synchronize()
                t0 = time.perf_counter()
                fn()
                flt.synchronize()
                if r:
                    times[k].append(time.perf_counter() - t0)
        for k, t in times.items():
            t.sort()
            med = t[len(t) // 2]
            out[k + "_us_per_frame"] = round(1e6 * med / N, 2)
            out[k + "_us_min_max"] = [round(1e6 * t[0] / N, 2), round(1e6 * t[-1] / N, 2)]
            out[k + "_GBps"] = round(3 * N * W * H * B / med / 1e9, 1)
            out[k + "_of_hbm_peak"] = round(3 * N * W * H * B / 8e12 / med, 3)
    return out


def merge_bandwidth(clip, a):
    """sn_merge_device against sn_mask_merge_device (expand 1, into a third plane), both on noise and moving 3 W H B bytes per
    frame, and sn_turn_merge_device (3 W H B) against sn_turn_device (2 W H B), alternating: median, minimum and maximum
    microseconds per frame over --reps launches of --frames frames; `of_hbm_peak` is the bytes over 8 TB/s over the median."""
    dev = torch.device("cuda:0")
    N, W, H, B = a.frames, clip.width, clip.height, clip.bytes
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.float32}[B]

    def noise():
        if B == 4:
            return torch.rand((N, H, W), device=dev)
        return torch.randint(0, 1 << clip.bits, (N, H, W), device=dev, dtype=torch.int32).to(dt)
    S, R = noise(), noise()
    dst = torch.empty((N, H, W), device=dev, dtype=dt)
    turned = torch.empty((N, W, H), device=dev, dtype=dt)
    lo, hi, _ = a.mask_values
    out = {"clip": f"{a.fmt} {W}x{H}", "frames": N, "plane_bytes": N * W * H * B, "mask": [lo, hi, 1], "reps": a.reps}
    with SangNom2(clip, max_batch=1) as flt:
        runs = {"merge": (3, lambda: flt.merge(S, R, dst)), "merge_in_place": (3, lambda: flt.merge(dst, R, dst)),
                "mask1": (3, lambda: flt.mask_merge(S, R, dst, lo, hi, 1)),
                "turn_merge": (3, lambda: flt.turn_merge(S, R, turned, 1)), "turn": (2, lambda: flt.turn(S, turned, 1))}
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        for r in range(a.reps + 1):
            for k, (_, fn) in runs.items():
                flt.synchronize()
                t0 = time.perf_counter()
                fn()
                flt.synchronize()
                if r:
                    times[k].append(time.perf_counter() - t0)
        for k, t in times.items():
            t.sort()
            med, moved = t[len(t) // 2], runs[k][0] * N * W * H * B
            out[k + "_us_per_frame"] = round(1e6 * med / N, 2)
            out[k + "_us_min_max"] = [round(1e6 * t[0] / N, 2), round(1e6 * t[-1] / N, 2)]
            out[k + "_GBps"] = round(moved / med / 1e9, 1)
            out[k + "_of_hbm_peak"] = round(moved / 8e12 / med, 3)
    return out


def fields_rates(clip, a, src, dst, kw):
    """The call with both fields next to the one-field call with the same other options, on the same frames, alternating:
    median, minimum and maximum frames/s over --reps batches of --frames frames each, and the ratio of the median times."""
    N = a.frames
    common = dict(max_batch=N, fresh_pool=bool(a.fresh), aac=48 if clip.planes > 1 else 0, **kw)
    with SangNomAA(clip, **common) as one, SangNomAA(clip, fields="both", **common) as both:
        ctx = {"one": one, "both": both}
        times = {k: [] for k in ctx}
        torch.cuda.synchronize()
        for r in range(a.reps + 2):  # two rounds of warm-up
            for k, aa in ctx.items():
                aa.synchronize()
                t0 = time.perf_counter()
                aa.process_batch(src, dst)
                aa.synchronize()
                if r >= 2:
                    times[k].append(time.perf_counter() - t0)
    out = {}
    for k, t in times.items():
        t.sort()
        out[f"aa_{k}_fps"] = round(N / t[len(t) // 2], 1)
        out[f"aa_{k}_fps_min_max"] = [round(N / t[-1], 1), round(N / t[0], 1)]
    out["both_over_one"] = round(times["both"][len(times["both"]) // 2] / times["one"][len(times["one"]) // 2], 3)
    return out


def luma_merge_times(clip, a, dev, dt, noise):
    """The chroma merge of a 4:2:0 frame whose luma plane is --size, in place on the result as the call uses it, expand 1, on
    noise: U and V through luma's mask in one launch (4 + 6 chroma-plane units of bytes: luma read, S and R read and dst
    written twice), in two launches (14 units), and the two own-mask merges (6 units); alternating, microseconds per frame."""
    N, W, H, B = a.frames, clip.width, clip.height, clip.bytes
    lo, hi, _ = a.mask_values
    L = noise(H, W)
    S, R = [noise(H // 2, W // 2) for _ in range(2)], [noise(H // 2, W // 2) for _ in range(2)]
    unit = N * (W // 2) * (H // 2) * B
    out = {}
    with SangNom2(clip, max_batch=1) as flt:
        def two():
            for p in range(2):
                flt.mask_merge_luma(L, S[p], R[p], R[p], lo, hi, 1)

        def own():
            for p in range(2):
                flt.mask_merge(S[p], R[p], R[p], lo, hi, 1)
        runs = {"luma_uv_one_launch": (10, lambda: flt.mask_merge_luma(L, S, R, R, lo, hi, 1)), "luma_uv_two_launches": (14, two), "own_uv": (6, own)}
        times = {k: [] for k in runs}
        torch.cuda.synchronize()
        for r in range(a.reps + 1):
            for k, (_, fn) in runs.items():
                flt.synchronize()
                t0 = time.perf_counter()
                fn()
                flt.synchronize()
                if r:
                    times[k].append(time.perf_counter() - t0)
        for k, t in times.items():
            t.sort()
            out[k + "_us_per_frame"] = round(1e6 * t[len(t) // 2] / N, 2)
            out[k + "_GBps"] = round(runs[k][0] * unit / t[len(t) // 2] / 1e9, 1)
            out[k + "_us_min_max"] = [round(1e6 * t[0] / N, 2), round(1e6 * t[-1] / N, 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--fresh", type=int, default=1)
    ap.add_argument("--fmt", default="Y8")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--host", action="store_true", help="frames from host memory: the synchronous call against the ring")
    ap.add_argument("--depth", type=int, default=8, help="--host: slots of the ring")
    ap.add_argument("--dh", action="store_true", help="both passes with dh=true: enlargement by two in both directions")
    ap.add_argument("--composed", action="store_true", help="--dh, device-resident: two SangNom2(dh=True) contexts and SangNom2.turn by hand")
    ap.add_argument("--reduce", choices=["tent", "halfband"], help="with dh: reduce the enlarged frame on the device (implies --dh)")
    ap.add_argument("--reduce-bw", action="store_true", help="the reduce kernel alone against the turn kernel on the same planes")
    ap.add_argument("--reps", type=int, default=9, help="--reduce-bw, --mask-bw: timed launches per kernel")
    ap.add_argument("--mask", help="lo,hi[,expand]: the call with the edge mask next to the call without it (at source size)")
    ap.add_argument("--mask-chroma", choices=["own", "luma"], default="own", help="--mask: which mask merges chroma (luma: the luma plane's, reduced)")
    ap.add_argument("--mask-bw", action="store_true", help="the mask kernel alone against the half-band reduce kernel on the same plane")
    ap.add_argument("--sharpen", type=int, default=0, help="AMOUNT 1..255: the call with the contra-sharpening next to the call without it (at source size)")
    ap.add_argument("--sharpen-chroma", action="store_true", help="--sharpen: every processed plane, not luma alone")
    ap.add_argument("--sharpen-bw", action="store_true", help="the sharpening kernel alone against the mask kernel on the same planes")
    ap.add_argument("--fields", choices=["one", "both"], default="one", help="both: the both-fields call next to the one-field call, alternating")
    ap.add_argument("--merge-bw", action="store_true", help="the averaging kernel alone against the mask kernel, and the turn of the average against the turn")
    ap.add_argument("--repair", type=int, default=0, help="K 1..4: the call with the rank repair next to the call without it (at source size)")
    ap.add_argument("--repair-chroma", action="store_true", help="--repair: every processed plane, not luma alone")
    ap.add_argument("--repair-bw", action="store_true", help="the repair kernel alone against the mask and sharpening kernels on the same planes")
    a = ap.parse_args()
    a.mask_values = ([int(x) for x in a.mask.split(",")] + [1])[:3] if a.mask else [8, 32, 1]
    mask_kw = dict(mask=tuple(a.mask_values[:2]), mask_expand=a.mask_values[2]) if a.mask else None
    if mask_kw and a.mask_chroma != "own":
        mask_kw["mask_chroma"] = a.mask_chroma
    w, h = [int(x) for x in a.size.split("x")]
    clip = clip_format(a.fmt, w, h)
    if a.reduce:
        a.dh = True
    if a.reduce_bw:
        print(json.dumps(reduce_bandwidth(clip, a)))
        return
    if a.mask_bw:
        print(json.dumps(mask_bandwidth(clip, a)))
        return
    if a.sharpen_bw:
        print(json.dumps(sharpen_bandwidth(clip, a)))
        return
    if a.merge_bw:
        print(json.dumps(merge_bandwidth(clip, a)))
        return
    if a.repair_bw:
        print(json.dumps(repair_bandwidth(clip, a)))
        return
    if clip.bytes != 1:
        sys.exit("aa_bench: 8-bit formats only")
    if a.fields == "both" and (a.dh or a.composed or a.host):
        sys.exit("aa_bench: --fields both goes without --dh, on device batches")
    if a.sharpen and ((a.dh and not a.reduce) or a.composed or a.host):
        sys.exit("aa_bench: --sharpen needs the frame at source size (without --dh, or with --reduce) and device batches")
    if a.repair and ((a.dh and not a.reduce) or a.composed or a.host or a.fields == "both"):
        sys.exit("aa_bench: --repair needs the frame at source size (without --dh, or with --reduce) and device batches of one field")
    if a.mask and ((a.dh and not a.reduce) or a.composed):
        sys.exit("aa_bench: --mask needs the frame at source size: without --dh, or with --reduce")
    if a.composed and (not a.dh or a.host or a.reduce):
        sys.exit("aa_bench: --composed goes with --dh, device-resident, without --reduce")
    if a.host:
        out = host_rates(clip, a)
        if a.mask:
            masked = host_rates(clip, a, mask_kw)
            out["mask"] = a.mask_values
            out.update({"mask_" + k: masked[k] for k in ("sync_fps", "ring_fps") if k in masked})
        print(json.dumps(out))
        return
    dev = torch.device("cuda:0")
    N = a.frames
    src = [torch.randint(0, 256, (N, h >> (clip.subh if p else 0), w >> (clip.subw if p else 0)), device=dev, dtype=torch.uint8)
           for p in range(clip.planes)]
    k = 2 if a.dh and not a.reduce else 1
    dst = [torch.empty((N, k * s.shape[1], k * s.shape[2]), device=dev, dtype=torch.uint8) for s in src]
    out = {"clip": f"{a.fmt} {w}x{h}", "frames": N, "fresh_pool": bool(a.fresh)}
    if a.dh:
        out["dh"] = True
    if a.reduce:
        out["reduce"] = a.reduce
    if a.composed:
        out["composed_fps"] = composed_dh_rate(clip, a, src, dst)
        print(json.dumps(out))
        return
    if a.fields == "both":
        kw = dict(mask_kw or {}, **(dict(sharpen=a.sharpen, sharpen_chroma=a.sharpen_chroma) if a.sharpen else {}))
        out.update(reps=a.reps, **({"mask": a.mask_values} if a.mask else {}), **({"sharpen": a.sharpen} if a.sharpen else {}))
        out.update(fields_rates(clip, a, src, dst, kw))
        print(json.dumps(out))
        return
    reps = 5
    sharpen_kw = dict(mask_kw or {}, sharpen=a.sharpen, sharpen_chroma=a.sharpen_chroma)
    before_repair = dict(sharpen_kw if a.sharpen else mask_kw or {})
    repair_kw = dict(before_repair, repair=a.repair, repair_chroma=a.repair_chroma)
    for key, kw in [("aa_fps", {})] + ([("aa_mask_fps", mask_kw)] if a.mask else []) + ([("aa_sharpen_fps", sharpen_kw)] if a.sharpen else []) + \
            ([("aa_repair_fps", repair_kw)] if a.repair else []):
        with SangNomAA(clip, max_batch=N, fresh_pool=bool(a.fresh), aac=48 if clip.planes > 1 else 0, **(dict(dh=True) if a.dh else {}),
                       **(dict(reduce=a.reduce) if a.reduce else {}), **kw) as aa:
            torch.cuda.synchronize()
            for _ in range(2):
                aa.process_batch(src, dst)
            aa.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                aa.process_batch(src, dst)
            aa.synchronize()
            out[key] = round(N * reps / (time.perf_counter() - t0), 1)
    if a.mask:
        out["mask"] = a.mask_values
        out["mask_chroma"] = a.mask_chroma
        out["mask_us_per_frame"] = round(1e6 / out["aa_mask_fps"] - 1e6 / out["aa_fps"], 2)
    if a.sharpen:  # on top of the mask where one is given
        out["sharpen"] = [a.sharpen, int(a.sharpen_chroma)]
        out["sharpen_us_per_frame"] = round(1e6 / out["aa_sharpen_fps"] - 1e6 / out["aa_mask_fps" if a.mask else "aa_fps"], 2)
    if a.repair:  # on top of the sharpening and the mask where given
        out["repair"] = [a.repair, int(a.repair_chroma)]
        out["repair_us_per_frame"] = round(1e6 / out["aa_repair_fps"] - 1e6 / out["aa_sharpen_fps" if a.sharpen else "aa_mask_fps" if a.mask else "aa_fps"], 2)
    with SangNom2(clip, max_batch=N) as flt:
        t = torch.empty((N, w, h), device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        flt.turn(src[0], t, 1)
        flt.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            flt.turn(src[0], t, 1)
        flt.synchronize()
        dt = (time.perf_counter() - t0) / reps
        out["turn_fps"] = round(N / dt, 1)
        out["turn_GBps"] = round(2 * N * w * h / dt / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
