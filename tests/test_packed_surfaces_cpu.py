"""Packed 4:2:2 surfaces without a GPU: the numpy model of the layouts the GPU tests trust (tests/packed_surface_cases.py)
against bytes and words written out by hand, the case table's own promises, the layout description the host walk uses
(csrc/sn_surface_layout.h, checked by a stand-alone program, once more under AddressSanitizer and UBSan) and the ctypes mirror."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import capi, clip_format, synth
from tests import msb_surface_cases as mc
from tests import packed_surface_cases as pc
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planes(clip, seed):
    return synth.frame(clip, "noise", seed=seed)


@pytest.mark.parametrize("w", [96, 98, 100, 64])
@pytest.mark.parametrize("layout,fmt", [("yuyv", "YUV422P8"), ("uyvy", "YUV422P8"), ("yuyv", "YUV422P16"), ("yuyv_msb", "YUV422P10"),
                                        ("uyvy_msb", "YUV422P12"), ("v210", "YUV422P10")])
def test_round_trips(layout, fmt, w):
    """unpack(pack(frame)) is the frame for destination packing and for a source with junk; the junk is really there."""
    clip = clip_format(fmt, w, 6)
    fr = _planes(clip, 31 + w)
    clean, junk = pc.pack_frames(layout, clip, [fr])[0], pc.pack_frames(layout, clip, [fr], source=True)[0]
    assert clean.shape == junk.shape == (6, pc.row_bytes(layout, w, clip.bytes) // clean.dtype.itemsize)
    assert clean.dtype == pc.packed_dtype(layout, clip)
    for packed in (clean, junk):
        back = pc.unpack_frames(layout, clip, [packed])[0]
        assert all(same(a, b) for a, b in zip(fr, back))
    if layout == "v210":
        assert np.all(clean >> 30 == 0) and np.any(junk >> 30 != 0)
        if w % 6:
            assert not same(clean[:, -4:], junk[:, -4:] & 0x3FFFFFFF)  # the fields of pixels >= w
    elif pc.is_msb(layout) and mc.shift_of(clip):
        low = (1 << mc.shift_of(clip)) - 1
        assert np.all(clean & low == 0) and np.all(junk & low != 0)
    else:
        assert same(clean, junk)


def test_yuyv_and_uyvy_known_answers():
    y, u, v = np.array([[0x10, 0x11, 0x12, 0x13]], np.uint8), np.array([[0x80, 0x81]], np.uint8), np.array([[0xF0, 0xF1]], np.uint8)
    assert pc.pack_yuyv(y, u, v, "yuyv").tobytes() == bytes([0x10, 0x80, 0x11, 0xF0, 0x12, 0x81, 0x13, 0xF1])
    assert pc.pack_yuyv(y, u, v, "uyvy").tobytes() == bytes([0x80, 0x10, 0xF0, 0x11, 0x81, 0x12, 0xF1, 0x13])
    clip = clip_format("YUV422P10", 2, 1)
    fr = [np.array([[0x3FF, 0x001]], np.uint16), np.array([[0x155]], np.uint16), np.array([[0x2AA]], np.uint16)]
    # Y210: every sample << 6, little-endian 16-bit words Y0 U0 Y1 V0
    assert pc.pack_frames("yuyv_msb", clip, [fr])[0].tobytes() == bytes([0xC0, 0xFF, 0x40, 0x55, 0x40, 0x00, 0x80, 0xAA])
    assert pc.pack_frames("uyvy_msb", clip, [fr])[0].tobytes() == bytes([0x40, 0x55, 0xC0, 0xFF, 0x80, 0xAA, 0x40, 0x00])
    # a sample above the range loses its high bits in the 16-bit word
    over = [np.array([[1087, 0]], np.uint16), fr[1], fr[2]]
    assert int(pc.pack_frames("yuyv_msb", clip, [over])[0][0, 0]) == (1087 << 6) & 0xFFFF == 4032


def test_v210_known_answers():
    y = np.array([[0x101, 0x102, 0x103, 0x104, 0x105, 0x106]], np.uint16)
    u, v = np.array([[0x201, 0x202, 0x203]], np.uint16), np.array([[0x301, 0x302, 0x303]], np.uint16)
    # word 0 = U0 | Y0 << 10 | V0 << 20, word 1 = Y1 | U1 << 10 | Y2 << 20, word 2 = V1 | Y3 << 10 | U2 << 20, word 3 = Y4 | V2 << 10 | Y5 << 20
    want = [0x201 | 0x101 << 10 | 0x301 << 20, 0x102 | 0x202 << 10 | 0x103 << 20, 0x302 | 0x104 << 10 | 0x203 << 20, 0x105 | 0x303 << 10 | 0x106 << 20]
    assert want == [0x30140601, 0x10380902, 0x20341302, 0x106C0D05]
    assert pc.pack_v210(y, u, v).tolist() == [want]
    # 4 pixels: Y4, V2, Y5 and U2 are zero fields; 2 pixels: only word 0 and Y1 of word 1 are left
    assert pc.pack_v210(y[:, :4], u[:, :2], v[:, :2]).tolist() == [[want[0], want[1], 0x302 | 0x104 << 10, 0]]
    assert pc.pack_v210(y[:, :2], u[:, :1], v[:, :1]).tolist() == [[want[0], 0x102, 0, 0]]
    # the mask: 1087 = 0x43F is packed as 0x03F
    assert pc.pack_v210(np.array([[1087, 0]], np.uint16), u[:, :1], v[:, :1]).tolist() == [[0x201 | 0x03F << 10 | 0x301 << 20, 0, 0, 0]]
    # junk in bits 30-31 and in the fields of missing pixels is ignored
    spoiled = np.array([[want[0] | 0xC0000000, 0x102 | 0x3FF << 10 | 0x3FF << 20 | 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF]], np.uint32)
    got = pc.unpack_v210(spoiled, 2)
    assert got[0].tolist() == [[0x101, 0x102]] and got[1].tolist() == [[0x201]] and got[2].tolist() == [[0x301]]
    assert pc.v210_blocks(96) == 16 and pc.v210_blocks(98) == 17 and pc.row_bytes("v210", 100, 2) == 272


def test_the_case_table_keeps_its_promises():
    """Every width class of the kernels is there; the out-of-range case really has samples above 2^bits - 1 (chosen by this
    assertion), so the v210 mask and the MSB shift drop bits that are set."""
    v210 = [c.w for c, layout in pc.PARITY if layout == "v210"]
    assert {w % 6 for w in v210} == {0, 2, 4} and any(w // 48 > 64 for w in v210) and any(w % 48 for w in v210)
    assert any(c.w // 32 > 128 for c, layout in pc.PARITY if layout == "yuyv")
    assert {layout for _, layout in pc.PARITY} == set(pc.LAYOUTS)
    clip, frames, par, want = pc.expected(pc.OUT_OF_RANGE)
    assert pc.exceeds_range(clip, want) and not pc.exceeds_range(clip, frames)
    for layout in pc.OUT_OF_RANGE_LAYOUTS:
        back = pc.unpack_frames(layout, clip, pc.pack_frames(layout, clip, want))
        assert not all(same(a, b) for fa, fb in zip(want, back) for a, b in zip(fa, fb)), layout


def test_scratch_formula_by_hand():
    clip = clip_format("YUV422P10", 100, 40)
    # pitches: luma 200 -> 256, chroma 100 -> 256
    assert pc.scratch_frame_bytes(clip, "v210", "v210") == (256 + 2 * 256) * 40 * 2
    assert pc.scratch_frame_bytes(clip, "v210", "planar") == (256 + 2 * 256) * 40
    assert pc.scratch_frame_bytes(clip, "planar", "v210") == (256 + 2 * 256) * 40
    assert pc.scratch_frame_bytes(clip, "planar_msb", "v210") == (256 + 2 * 256) * 40 * 2
    assert pc.scratch_frame_bytes(clip, "nv16", "yuyv_msb") == (2 * 256) * 40 + (256 + 2 * 256) * 40
    assert pc.scratch_frame_bytes(clip, "yuyv_msb", "nv16") == (256 + 2 * 256) * 40 + (2 * 256) * 40
    assert pc.scratch_frame_bytes(clip, "v210", "v210", dh=True) == (256 + 2 * 256) * 40 * 3
    assert pc.scratch_frame_bytes(clip, "v210", "v210", dh=True, aa=True) == (256 + 2 * 256) * 40 + (512 + 2 * 256) * 80


def _build_layout_check(tmp_path, name, extra):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc"), *extra,
                           os.path.join(ROOT, "tests", "c", "surface_layout_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_layout_description_matches_values_written_out_by_hand(tmp_path, sanitized):
    """sn::surface_layout and its companions (csrc/sn_surface_layout.h): row bytes, alignment units, the planes that must be NULL
    and the refusal table, against tests/c/surface_layout_check.cpp.  A host compiler takes the header as it is; the second
    build runs the same stand-alone program under AddressSanitizer and UBSan."""
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    exe = _build_layout_check(tmp_path, "surface_layout_check" + ("_san" if sanitized else ""), extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])


def test_ctypes_mirror():
    assert (capi.SN_LAYOUT_PACKED_YUYV, capi.SN_LAYOUT_PACKED_UYVY, capi.SN_LAYOUT_PACKED_YUYV_MSB, capi.SN_LAYOUT_PACKED_UYVY_MSB,
            capi.SN_LAYOUT_PACKED_V210) == (8, 9, 10, 11, 12)
    assert capi.PACKED_LAYOUTS[("yuyv", True)] == 10 and ("v210", True) not in capi.PACKED_LAYOUTS
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in ("PACKED_YUYV", "PACKED_UYVY", "PACKED_YUYV_MSB", "PACKED_UYVY_MSB", "PACKED_V210"):
        assert f"SN_LAYOUT_{name} = {getattr(capi, 'SN_LAYOUT_' + name)}" in header
    s = capi.surfaces(capi.SN_LAYOUT_PACKED_V210, [0x1000], [272], [272 * 40])
    assert s.struct_size == ctypes.sizeof(capi.SnSurfaces) and s.layout == 12
    assert (s.plane[0], s.plane[1], s.plane[2]) == (0x1000, None, None)
    assert (s.pitch[0], s.frame_stride[0], s.reserved) == (272, 272 * 40, 0)


def test_formats_and_keywords():
    from avisynth_sangnom2_amd import SangNom2, SangNomAA
    import inspect
    for fmt, bits in (("YUV422P10", 10), ("YUV422P12", 12)):
        clip = clip_format(fmt, 64, 16)
        assert (clip.bytes, clip.bits, clip.planes, clip.subw, clip.subh) == (2, bits, 3, 1, 0)
    for cls in (SangNom2, SangNomAA):
        p = inspect.signature(cls.process_surfaces).parameters
        assert p["src_packed"].default is None and p["dst_packed"].default is None
