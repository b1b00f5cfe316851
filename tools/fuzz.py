#!/usr/bin/env python3
"""Randomised parity run on the GPU: random formats, sizes, arguments, extension flags and frame sequences through
the C ABI (host frames, device batches and the host ring) against oracle instances.  A quarter of the integer
configurations run with opt=1 (the SSE2 arithmetic, against tests/sse2_model.py), and those draw sn_policy.sse2_sweeps too.
Wide 16-bit and float configurations (3872 .. 8192 columns) draw sn_options.column_parts.
Device batches of three-plane 8 / 16-bit clips draw the layout of each side: planar, or semi-planar (a UV plane; sn_process_device_surfaces).
Device batches of 9..15-bit clips also draw each side's alignment: LSB, or MSB (P010 / P012: the sample in the high bits, random low bits below it).
Device batches of 4:2:2 8 / 16-bit clips draw a packed layout for each side as well (YUYV / UYVY, their MSB forms, v210 on 10-bit clips; junk where a source may carry it).
usage: python tools/fuzz.py [--seconds 120] [--seed 1]"""
import argparse
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avisynth_sangnom2_amd import SangNom2, clip_format, synth  # noqa: E402
from tests import packed_surface_cases as pc  # noqa: E402
from tests.config_space import cfg_of, compose, reference  # noqa: E402,F401  (the reference's composition, shared with the covering table)
from tests.util import to_host  # noqa: E402

FORMATS = ["Y8", "Y8", "Y8", "Y10", "Y16", "Y32", "YUV420P8", "YUV420P8", "YUV420P16", "YUV422P8", "YUV444P8", "YUV444PS", "YUV420PS", "YUV420P10",
           "YUV420P12", "YUV422P10", "YUV422P10", "YUV422P12", "YUV422P16"]


def same(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


CURRENT = [""]  # the configuration under way, for the report when a call raises


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = random.Random(a.seed)
    t_end = time.time() + a.seconds
    n = bad = 0
    stats = {"fused": 0, "pool": 0, "ring": 0, "host": 0, "batch": 0, "frames": 0, "pixels": 0, "banded_frames": 0, "band_fallbacks": 0, "chained_frames": 0,
             "uv_sweep_configs": 0, "chain_redone": 0, "opt1": 0, "opt1_sweeps": 0, "part_frames": 0, "part_fallbacks": 0, "semi_sides": 0, "msb_sides": 0, "packed_sides": 0}
    while time.time() < t_end:
        fmt = rng.choice(FORMATS)
        wide = rng.random() < 0.15
        w = rng.choice([32, 64, 96, 128, 160, 256, 320, 512, 544, 640, 992, 1024]) if not wide else rng.choice([1472, 1920, 1952, 2048, 2432, 2880, 3840, 4096, 5120, 7680])
        if rng.random() < 0.25:
            w = rng.choice([40, 72, 100, 200, 360, 720, 1080]) if not wide else 2160  # not a multiple of 32
        h = 2 * rng.randint(1, 40 if not wide else 12)
        if rng.random() < 0.3:
            h = 2 * rng.randint(20, 200 if not wide else 60)  # tall enough for the row bands of the latency path
            if rng.random() < 0.15:
                h = 2 * rng.randint(200, 540)  # ... and for the hand-off's dependency cone to reach the last columns
        probe = clip_format(fmt, 64, 32)
        if probe.planes == 3:
            w -= w % (4 if probe.subw else 1) or 0
            if probe.subh:
                h += (-h) % 4
            if probe.subw and (w // 2) % 2:
                w += 2
        if probe.bytes > 1 and w > 3840 and rng.random() < 0.7:
            w = 3840
        # 16-bit and float planes wider than one workgroup of the sweeps: now and then in column parts (sn_options.column_parts)
        column_parts = 0
        if probe.bytes > 1 and wide and rng.random() < 0.5:
            w = rng.choice([3872, 4096, 5120, 6144, 7680, 8192])
            column_parts = 1
        clip = clip_format(fmt, w, h)
        kw = dict(order=rng.randint(0, 2), aa=rng.choice([0, 1, 20, 48, 100, 128]), aac=rng.choice([0, 48, 128]),
                  dh=rng.random() < 0.2, luma=rng.random() < 0.85, chroma=rng.random() < 0.8)
        ext = rng.choice(["none", "none", "isolated", "fresh"])
        way = rng.choice(["host", "ring", "batch"])  # batch: device-resident frames, one launch (history-carrying 8-bit clips: the chain)
        nframes = rng.randint(1, 4) if way != "batch" else rng.randint(2, 10)
        opt = 1 if clip.bytes < 4 and rng.random() < 0.25 else 0
        knob = rng.choice([0, 1]) if opt == 1 else 0  # sn_policy.sse2_sweeps: which kernels run in the SSE2 arithmetic
        if opt == 1 and min(w >> (clip.subw if p else 0) for p in range(clip.planes)) < 32 // clip.bytes:
            continue  # the SSE2 path is defined from two vectors per row on
        pattern = rng.choice(["noise", "noise", "checker", "edges", "sine"] + (["noise01", "noise01", "checker2"] if opt == 1 else []))
        frames = [synth.frame(clip, pattern, seed=rng.randint(0, 1 << 20)) for _ in range(nframes)]
        parity = [rng.randint(0, 1) for _ in range(nframes)]
        want = compose(clip, frames, parity, kw, ext, opt)  # expected
        CURRENT[0] = f"{fmt} {w}x{h} {kw} ext={ext} way={way} nframes={nframes} opt={opt} sse2_sweeps={knob} column_parts={column_parts} pattern={pattern}"
        small = rng.choice([1, 0])  # SN_SMALL_SWEEP: the whole-plane sweeps, or auto mode's small-launch paths (bands, pool kernels)
        try:
            sweeps = rng.choice([0, 0, 0, 1])  # 8-bit 4:2:0: U and V as one sweep (default) or a sweep each
            flt = SangNom2(clip, host_depth=rng.choice([1, 2, 3, 4, 5, 8, 12]), max_batch=nframes, isolated_planes=ext == "isolated", fresh_pool=ext == "fresh", small_launches=small,
                           chroma_sweeps=sweeps, opt=opt, sse2_sweeps=knob, column_parts=column_parts, **kw)
        except Exception as e:  # a geometry the library rejects must be one it documents
            if "exceeds the supported maximum" in str(e):
                continue
            raise
        with flt:
            band_set = None
            if small == 0:  # auto mode: the row bands too, now and then with a run-up that is too short
                band_set = (rng.choice([0, 0, 2, 3, 5, 9, 16]), rng.choice([0, 0, 0, 1, 6, 12]))
                flt.set_bands(*band_set)
            got = []
            fused = False
            stats[way] += 1
            stats["frames"] += nframes
            stats["pixels"] += nframes * w * h
            if way == "host":
                got = [flt.get_frame(frames[f], parity=parity[f]) for f in range(nframes)]
            elif way == "batch":
                import torch
                dev = torch.device("cuda:0")
                view = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]
                # 9..15-bit clips: each side LSB- or MSB-aligned, independently; an MSB source has random low bits, which must not matter
                shift = 16 - clip.bits if clip.bytes == 2 else 0
                msb_in, msb_out = (rng.random() < 0.5, rng.random() < 0.5) if shift else (False, False)
                words = frames
                if msb_in:
                    low = np.random.default_rng(rng.randint(0, 1 << 30))
                    words = [[(pl << np.uint16(shift)) | low.integers(0, 1 << shift, pl.shape, dtype=np.uint16) for pl in fr] for fr in frames]
                src = [torch.from_numpy(np.stack([fr[p] for fr in words]).view(view)).to(dev) for p in range(clip.planes)]
                dst = [torch.zeros((nframes,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
                # three-plane 8 / 16-bit clips: each side planar or semi-planar (NV12 / P016 / NV16 / NV24), independently
                semi_in, semi_out = (rng.random() < 0.5, rng.random() < 0.5) if clip.planes == 3 and clip.bytes < 4 else (False, False)
                if semi_in:
                    src = [src[0], torch.stack([src[1], src[2]], dim=-1).contiguous()]
                if semi_out:
                    dst = [dst[0], torch.zeros(tuple(dst[1].shape) + (2,), dtype=dst[1].dtype, device=dev)]
                # 4:2:2 8 / 16-bit clips: each side may be ONE packed plane instead (tests/packed_surface_cases.py has the numpy model)
                packed_in = packed_out = None
                if clip.planes == 3 and (clip.subw, clip.subh) == (1, 0) and clip.bytes < 4:
                    kinds = ["yuyv", "uyvy"] + (["yuyv_msb", "uyvy_msb"] if clip.bytes == 2 else []) + (["v210", "v210"] if clip.bits == 10 else [])
                    packed_in, packed_out = (rng.choice(kinds) if rng.random() < 0.5 else None for _ in range(2))
                pview = {1: np.uint8, 2: np.int16, 4: np.int32}
                if packed_in:
                    rows = np.stack(pc.pack_frames(packed_in, clip, frames, source=True, seed=rng.randint(0, 1 << 20)))  # (not `a`: the arguments)
                    src, semi_in, msb_in = torch.from_numpy(rows.view(pview[rows.dtype.itemsize])).to(dev), False, pc.is_msb(packed_in)
                if packed_out:
                    oh, ow = flt.plane_shape_out(0)
                    shape = (nframes, oh, 4 * pc.v210_blocks(ow)) if packed_out == "v210" else (nframes, oh, 2 * ow)
                    dst = torch.zeros(shape, dtype=torch.int32 if packed_out == "v210" else {1: torch.uint8, 2: torch.int16}[clip.bytes], device=dev)
                    semi_out, msb_out = False, pc.is_msb(packed_out)
                stats["semi_sides"] += int(semi_in) + int(semi_out)
                stats["msb_sides"] += int(msb_in) + int(msb_out)
                stats["packed_sides"] += int(bool(packed_in)) + int(bool(packed_out))
                torch.cuda.synchronize()
                if semi_in or semi_out or msb_in or msb_out or packed_in or packed_out or rng.random() < 0.25:
                    flt.process_surfaces(src, dst, parity=parity, src_msb=msb_in, dst_msb=msb_out, src_packed=packed_in and pc.order_of(packed_in),
                                         dst_packed=packed_out and pc.order_of(packed_out))
                else:
                    flt.process_batch(src, dst, parity=parity)
                flt.synchronize()
                if packed_out:  # both sides of the comparison as planar LSB planes of the output's size, the bits a packed word drops gone
                    oclip = clip_format(fmt, ow, oh)
                    got = pc.unpack_frames(packed_out, oclip, list(to_host(dst).view(pc.packed_dtype(packed_out, clip))))
                    want = pc.unpack_frames(packed_out, oclip, pc.pack_frames(packed_out, oclip, want))
                    msb_out = False
                elif semi_out:
                    dst = [dst[0], dst[1][..., 0], dst[1][..., 1]]
                if not packed_out:
                    got = [[to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)] for f in range(nframes)]
                if msb_out:  # the rule: the LSB result shifted left inside its 16-bit word
                    want = [[(pl << np.uint16(shift)).astype(np.uint16) for pl in fr] for fr in want]
            else:
                slots = flt.host_slots()
                inflight = []
                for f in range(nframes):
                    if len(inflight) == slots:
                        got.append(flt.collect(inflight.pop(0)))
                    inflight.append(flt.submit(frames[f], parity=parity[f]))
                while inflight:
                    got.append(flt.collect(inflight.pop(0)))
            info = flt.info()
            fused = info.fused_frames > 0
            stats["banded_frames"] += info.banded_frames
            stats["band_fallbacks"] += info.band_fallbacks
            stats["chained_frames"] += info.chained_frames
            stats["uv_sweep_configs"] += info.uv_sweeps
            stats["chain_redone"] += info.chain_redone
            stats["opt1"] += opt
            stats["opt1_sweeps"] += knob
            pinfo = flt.parts_info()
            stats["part_frames"] += pinfo.part_frames
            stats["part_fallbacks"] += pinfo.part_fallbacks
        stats["fused" if fused else "pool"] += 1
        for f in range(nframes):
            for p in range(clip.planes):
                if not same(want[f][p], got[f][p]):
                    bad += 1
                    d = np.argwhere(want[f][p] != got[f][p])
                    np.savez(f"gpurun_out/fuzz_mismatch_{n}.npz", **{f"src{q}": frames[f][q] for q in range(clip.planes)},
                             **{f"want{q}": want[f][q] for q in range(clip.planes)}, **{f"got{q}": got[f][q] for q in range(clip.planes)})
                    print(f"MISMATCH {fmt} {w}x{h} {kw} ext={ext} way={way} frame {f}/{nframes} plane {p} pattern={pattern} parity={parity} "
                          f"small_launches={small} chroma_sweeps={sweeps} opt={opt} sse2_sweeps={knob} column_parts={column_parts} part_frames={pinfo.part_frames} part_fallbacks={pinfo.part_fallbacks} uv={info.uv_sweeps} bands={band_set} banded={info.banded_frames} fallbacks={info.band_fallbacks} "
                          f"fused={info.fused_frames} n={len(d)} rows {d[:, 0].min()}..{d[:, 0].max()} cols {d[:, 1].min()}..{d[:, 1].max()}", flush=True)
        n += 1
        if n % 50 == 0:
            print(f"{n} configurations, {bad} mismatches", flush=True)
    print(f"fuzz: {n} configurations, {bad} mismatches (seed {a.seed}); {stats}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    try:
        main()
    except Exception:
        print(f"fuzz: a call raised in configuration: {CURRENT[0]}", flush=True)
        raise
